"""tests/background_ref.py (the definition of background subtraction in numpy) held to a plain-Python loop with a flood fill, and to
scipy.ndimage.label where that is importable; the hand-made cases' witnesses; the mutants the cases kill; the seeded generator's mix.  No GPU."""
import numpy as np
import pytest

from tests import background_cases as cases, background_ref as ref

CASES = cases.cases()


def python_run(maps, model, widths, heights, margin, rel_q, min_pixels):
    """The header's wording, pixel by pixel: -> (out, counts [T, n, 6], labels)."""
    maps = np.asarray(maps)
    T, px = maps.shape
    out = np.zeros((T, px), np.uint16)
    labels = np.full((T, px), -1, np.int64)
    counts = np.zeros((T, len(widths), 6), np.int64)
    for t in range(T):
        base = 0
        for f, (w, h) in enumerate(zip(widths, heights)):
            for i in range(w * h):
                c, lo = int(maps[t, base + i]), int(model[base + i])
                thr = margin + (lo * rel_q) // 1024
                if c != 0 and lo == 0:
                    out[t, base + i] = c
                    counts[t, f, ref.UNKNOWN] += 1
                elif c != 0 and c + thr < lo:
                    out[t, base + i] = c
                    counts[t, f, ref.FOREGROUND] += 1
                elif c != 0:
                    counts[t, f, ref.BACKGROUND] += 1
            if min_pixels >= 2:
                # flood fill in raster order: the first pixel that reaches a component is its lowest index
                for i in range(w * h):
                    if out[t, base + i] == 0 or labels[t, base + i] >= 0:
                        continue
                    stack, members = [i], []
                    labels[t, base + i] = i
                    while stack:
                        p = stack.pop()
                        members.append(p)
                        y, x = divmod(p, w)
                        for q, ok in ((p - 1, x > 0), (p + 1, x < w - 1), (p - w, y > 0), (p + w, y < h - 1)):
                            if ok and out[t, base + q] != 0 and labels[t, base + q] < 0:
                                labels[t, base + q] = i
                                stack.append(q)
                    counts[t, f, ref.COMPONENTS] += 1
                    if len(members) < min_pixels:
                        counts[t, f, ref.COMPONENTS_REMOVED] += 1
                        counts[t, f, ref.PIXELS_REMOVED] += len(members)
                        for p in members:
                            out[t, base + p] = 0
            base += w * h
    return out, counts, labels if min_pixels >= 2 else None


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[2] is None) == (b[2] is None) and (a[2] is None or np.array_equal(a[2], b[2]))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_made_cases_reach_what_they_are_named_for(case):
    got = case.want()
    case.witness(*got)
    assert same(got, python_run(case.maps, case.model, case.widths, case.heights, *case.params)), case.name


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS)
def test_seeded_rigs_have_every_kind_of_pixel_and_component(seed):
    """Kept, background and unknown pixels; with a blob pass a removed and a surviving component; a component across two tiles -- and the
    restatement equals the plain loop on the seed's first tick."""
    cases.fuzz_witness(seed)
    sizes, params, room, maps = cases.fuzz_case(seed)
    widths, heights = [s[0] for s in sizes], [s[1] for s in sizes]
    model = ref.learn(np.zeros(maps.shape[1], np.uint16), room)
    assert same(ref.run(maps[:1], model, widths, heights, *params), python_run(maps[:1], model, widths, heights, *params))


def test_the_generator_reaches_every_setting():
    params = [cases.fuzz_case(s)[1] for s in cases.FUZZ_SEEDS]
    assert {p[2] >= 2 for p in params} == {True, False} and len({p[0] for p in params}) >= 3 and {0, 255} <= {p[1] for p in params}
    assert {len(cases.fuzz_case(s)[0]) for s in cases.FUZZ_SEEDS} >= {1, 8}


def test_labels_equal_scipy_or_the_flood_fill():
    rng = np.random.default_rng(4)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for w, h in ((7, 5), (129, 17), (136, 40), (256, 64)):
        for density in (0.3, 0.55, 0.8):
            mask = rng.random((h, w)) < density
            lab = ref.labels_2d(mask)
            if ndimage is not None:
                sl, n = ndimage.label(mask)                        # 4-connectivity is scipy's default structure
                first = ndimage.minimum(np.arange(w * h).reshape(h, w), sl, np.arange(1, n + 1)).astype(np.int64)
                want = np.where(mask, first[np.maximum(sl, 1) - 1] if n else -1, -1)
            else:
                maps = np.where(mask, 9, 0).astype(np.uint16).reshape(1, -1)
                want = python_run(maps, np.zeros(w * h, np.uint16), [w], [h], 1, 0, 2)[2].reshape(h, w)
            assert np.array_equal(lab, want), (w, h, density)


def test_learning_is_order_independent_and_splits():
    rng = np.random.default_rng(8)
    maps = cases.learn_maps(rng, 500, 6)
    zero = np.zeros(500, np.uint16)
    whole = ref.learn(zero, maps)
    want = np.zeros(500, np.int64)
    for i in range(500):                                            # the plain loop
        for t in range(6):
            c = int(maps[t, i])
            if c != 0:
                want[i] = c if want[i] == 0 else min(want[i], c)
    assert np.array_equal(whole, want)
    assert np.array_equal(ref.learn(zero, maps[rng.permutation(6)]), whole)
    step = zero
    for t in range(6):
        step = ref.learn(step, maps[t:t + 1])
    assert np.array_equal(step, whole)
    assert np.array_equal(ref.learn(whole, np.zeros((3, 500), np.uint16)), whole) and (whole == 0).any() and (whole == 65535).any()


def _merged(case, how):
    """The case with its frames (one above the other) or its ticks read as ONE image: what a labelling that joins across them computes."""
    w = case.widths[0]
    if how == "frames":
        return ref.run(case.maps, case.model, [w], [sum(case.heights)], *case.params)[0]
    T = case.maps.shape[0]
    return ref.run(case.maps.reshape(1, -1), np.tile(case.model, T), [w], [T * case.heights[0]], *case.params)[0].reshape(T, -1)


MUTANTS = {
    "< against <=": lambda c: c.want(strict=False)[0],
    "thr without the floor": lambda c: c.want(floor=False)[0],
    "8- against 4-connectivity": lambda c: c.want(connectivity=8)[0] if c.params[2] >= 2 else c.want()[0],
    ">= against > on min_pixels": lambda c: c.want(at_least=False)[0] if c.params[2] >= 2 else c.want()[0],
    "joins across frames": lambda c: _merged(c, "frames") if len(set(c.widths)) == 1 and len(c.sizes) > 1 else c.want()[0],
    "joins across ticks": lambda c: _merged(c, "ticks") if len(c.sizes) == 1 and c.maps.shape[0] > 1 else c.want()[0],
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_cases_kill_the_mutant(mutant):
    killed = [c.name for c in CASES if not np.array_equal(MUTANTS[mutant](c), c.want()[0])]
    assert killed, mutant


def test_the_cases_kill_label_is_the_highest_index():
    """The maps do not show which member names a component; the labels do, and the plain loop holds them."""
    killed = [c.name for c in CASES if c.params[2] >= 2 and not np.array_equal(c.want(highest=True)[2], python_run(c.maps, c.model, c.widths, c.heights, *c.params)[2])]
    assert len(killed) >= 5, killed
