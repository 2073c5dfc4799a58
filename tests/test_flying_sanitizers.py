"""The host side of the flying-pixel filter under sanitizers, without a GPU: the ASan and TSan soak binaries of tests/fake_hip (built by
its Makefile as it is, see tests/test_host_sanitizers.py) run with $LSN_FLYING_PIXELS=1,20 -- alone, sharded over the double's two devices,
together with the outlier filter, and over a spread of $LSN_TEST_FAIL_ALLOC=n that reaches the new reservations (the lanes' filtered maps,
the plans' tile lists and per-tile counts: about 22 more allocations per two-iteration soak than with the switch off, interleaved with
the others from the first radial-first call on).  Under the runtime double the new kernel is a launch stub that does nothing, as the radial
kernels are: the soak's radial-first calls already expect an empty cloud, so its checks hold as they are; what this buys is the extents,
lifetimes and thread ordering of the new scratch and launches: clean sanitizers, an empty pool at the end."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ON = {"LSN_FLYING_PIXELS": "1,20"}


@pytest.fixture(scope="module")
def soaks():
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang is not installed here")
    r = subprocess.run(["make", "-C", FAKE, "-j4", "asan", "tsan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return {k: os.path.join(FAKE, "build", k, "soak") for k in ("asan", "tsan")}


def _run(binary, iters, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("LSN_")}
    e.update(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=0", **env)
    r = subprocess.run([binary, str(iters)], capture_output=True, text=True, env=e, timeout=600)
    text = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in text and "runtime error:" not in text and "WARNING: ThreadSanitizer" not in text, text[-4000:]
    assert "CHECK failed" not in text, text[-4000:]
    assert r.returncode == 0, text[-4000:]
    summary = [ln for ln in r.stdout.splitlines() if ln.startswith("soak:")]
    assert len(summary) == 1 and "pool 0 live" in summary[0] and "0 check(s) failed" in summary[0], text[-2000:]
    return summary[0]


def _fault_points(line):
    return int(line.split("fault points ")[1].split(",")[0])


@pytest.mark.parametrize("kind", ["asan", "tsan"])
@pytest.mark.parametrize("extra", [{}, {"LSN_OUTLIER_FILTER": "10,0.1"}], ids=["alone", "with-outlier-filter"])
def test_call_mix_with_the_switch_on(soaks, kind, extra):
    line = _run(soaks[kind], 3, **ON, **extra)
    assert "over 1 device part(s)" in line
    if kind == "asan" and not extra:
        # the switch reaches code that allocates: the run passes more allocation fault points than one with the switch off
        assert _fault_points(_run(soaks[kind], 2, **ON)) > _fault_points(_run(soaks[kind], 2)) + 10


@pytest.mark.parametrize("kind", ["asan", "tsan"])
@pytest.mark.parametrize("devices,parts,extra", [("0,1", 2, {}), ("0,1,1", 3, {}), ("0,1", 2, {"LSN_OUTLIER_FILTER": "10,0.1"})],
                         ids=["0,1", "0,1,1", "0,1-with-outlier-filter"])
def test_sharded_with_the_switch_on(soaks, kind, devices, parts, extra):
    """Every device filters its own block, in the tick as one call and in the sharded radial export (with the outlier filter on, the
    mesh call runs on the first device alone and filters there)."""
    line = _run(soaks[kind], 3, LSN_HOST_DEVICES=devices, **ON, **extra)
    assert f"over {parts} device part(s)" in line


@pytest.mark.parametrize("devices", ["", "0,1", "0,1,1"])
def test_failed_allocations_with_the_switch_on(soaks, devices):
    """Every early allocation and a spread over the rest of the run: the call that is hit returns nothing, everything after it works, the
    pool ends empty."""
    env = dict(ON)
    if devices:
        env["LSN_HOST_DEVICES"] = devices
    spread = list(range(1, 64)) + list(range(64, 560, 16)) if not devices else list(range(1, 720, 24))
    for n in spread:
        _run(soaks["asan"], 2, LSN_TEST_FAIL_ALLOC=str(n), **env)
    for n in (3, 17, 40, 90, 300):
        _run(soaks["tsan"], 2, LSN_TEST_FAIL_ALLOC=str(n), **env)
    both = dict(env, LSN_OUTLIER_FILTER="10,0.1")
    for n in (8, 20, 33, 47, 120, 350, 505, 700):
        _run(soaks["asan"], 2, LSN_TEST_FAIL_ALLOC=str(n), **both)
