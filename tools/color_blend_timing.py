#!/usr/bin/env python3
"""The colour blend (lsnFusionColorBlend) on 8 x 512x424 ring-scene ticks, a batch of `ticks` ticks (8 distinct ones, repeated) already in
HBM, with the colour transfer on the same plan in the same run as the yardstick.  One JSON line:

  blend_us_per_tick        HIP events round one lsnFusionColorBlend(20, 5) over all ticks (median of `reps`), per tick: the cloud index
                           (index pass, scan, confidence), the snapshot and the blend kernel
  transfer_us_per_tick     lsnFusionColorTransfer on the same plan, per tick (each rep from the untransferred cloud)
  vertices_per_tick, partner_terms_per_tick, blended_per_tick   from the stage's own counters (mean over the ticks)
  bytes_per_tick_at_least  what the two kernels need by the algorithm: 8 B a vertex for the snapshot (4 read, 4 written), 21 B a vertex for
                           the blend kernel's own loads (16 vertex, 4 pixel, 1 confidence), 7 B per projection that lands in a partner's
                           frame (2 depth, 1 confidence, 4 pixel -> vertex; counted here per partner TERM, a lower bound), 4 B per
                           partner term (its colour) and 4 B per blended vertex

The two kernels' own times come from a kernel trace of the --device-only run (tools/prof.sh).

With --quality (a synthetic figure; nobody has measured real Kinect frames): the ring scene with a gain and an offset per sensor on the
colour maps (tests/color_cases.py), one tick, through the definition's own partner test: the mean absolute colour difference, per
channel, between a vertex and each of its partner terms, before and after the blend, with and without the colour transfer in front.

    python tools/color_blend_timing.py [ticks] [reps] [--device-only] [--quality]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native  # noqa: E402
from tests import color_cases  # noqa: E402
from tools import timing  # noqa: E402

SETTING = (20, 5)


def _pair_difference(rig, orc, verts):
    """Mean |colour of a vertex - colour of its partner| per channel over all partner terms of the definition (setting SETTING)."""
    import numpy as np
    from tests import color_blend_ref as ref
    terms = []
    S = ref.sensors_of(rig, orc)
    ref.blend(rig, orc, *SETTING, verts=verts, sensors=S, terms=terms)
    _, off = ref.fused(S)
    C = np.stack([verts["R"], verts["G"], verts["B"]], axis=1).astype(np.int64)
    total = count = 0
    for t in terms:
        if t["i"] is None:
            continue
        ok = t["took_part"]
        own = C[off[t["j"]]:off[t["j"] + 1]][ok]
        other = C[off[t["i"]] + t["v"][ok]]
        total += int(np.abs(own - other).sum())
        count += 3 * int(ok.sum())
    return total / max(count, 1), count // 3


def quality():
    from oracle import orc
    from tests import color_blend_ref as ref, color_ref
    orc.build()
    rig = color_cases.ring(8)
    plain, _ = ref.fused(ref.sensors_of(rig, orc))
    moved, diag = color_ref.color_transfer(rig, orc)
    res = {"figure": "synthetic: ring scene, per-sensor colour gain and offset", "setting": SETTING, "transfer_pairs": len(diag["pairs"])}
    for label, start in (("plain", plain), ("after_transfer", moved)):
        before, n = _pair_difference(rig, orc, start)
        after, _ = _pair_difference(rig, orc, ref.blend(rig, orc, *SETTING, verts=start)[0])
        res[label] = {"partner_terms": n, "mean_abs_diff_before": round(before, 3), "mean_abs_diff_after": round(after, 3)}
    print(json.dumps(res))


def main():
    if "--quality" in sys.argv:
        return quality()
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    nums = [a for a in sys.argv[1:] if a.isdigit()]
    ticks, reps = (int(nums[i]) if len(nums) > i else d for i, d in enumerate((64, 10)))
    native.require_gpu()
    rigs = [color_cases.ring(8, tick=k) for k in range(min(ticks, 8))]
    with DeviceFusion.from_rigs(rigs, n_ticks=ticks) as fus:
        fus.run()
        blend = timing.event_ms(lambda: fus.color_blend(*SETTING), reps, 2, before=fus.run) * 1e3 / ticks
        res = {"rig": "8 x 512x424 ring scene", "ticks": ticks, "setting": SETTING, "blend_us_per_tick": round(blend, 2)}
        fus.run()
        fus.color_blend(*SETTING)
        torch.cuda.synchronize()
        d = [fus.color_blend_diagnostics(k) for k in range(min(ticks, 8))]
        nv = float(fus.host_offsets()[:len(d), -1].mean())
        terms, blended = (sum(float(x[key].sum()) for x in d) / len(d) for key in ("partners", "blended"))
        res.update(vertices_per_tick=round(nv), partner_terms_per_tick=round(terms), blended_per_tick=round(blended))
        # the projections that land in a partner's frame are not counted by the stage: the terms are a lower bound of them
        res["bytes_per_tick_at_least"] = round(nv * (8 + 21) + terms * (7 + 4) + blended * 4)
        if "--device-only" not in sys.argv:
            res["transfer_us_per_tick"] = round(timing.event_ms(fus.color_transfer, reps, 2, before=fus.run) * 1e3 / ticks, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
