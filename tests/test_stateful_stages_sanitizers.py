"""The host side of the two stages with state under sanitizers, without a GPU: the ASan and TSan soak binaries of tests/fake_hip (built by
its Makefile as it is, see tests/test_host_sanitizers.py) run with $LSN_TEMPORAL_FILTER=64,20,2 and $LSN_BACKGROUND=40,8,64,2 together --
on one device and sharded over the double's two, and over a spread of $LSN_TEST_FAIL_ALLOC=n that reaches the state records' reservations
(histories, models, filtered maps, count words, the blob pass's scratch) in the lanes and in the soak's `stateful_stages` case, which
drives the device-resident forms on a plan and on a tick object.  Under the runtime double the kernels are launch stubs that do nothing;
what this buys is the extents, lifetimes and thread ordering of the buffers and launches: clean sanitizers, an empty pool at the end.
Only the stand-alone soak programs run under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_hip")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ON = {"LSN_TEMPORAL_FILTER": "64,20,2", "LSN_BACKGROUND": "40,8,64,2"}


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
@pytest.mark.parametrize("devices,parts", [("", 1), ("0,1", 2)], ids=["one-device", "0,1"])
def test_call_mix_with_both_switches_on(soaks, kind, devices, parts):
    env = dict(ON)
    if devices:
        env["LSN_HOST_DEVICES"] = devices
    line = _run(soaks[kind], 3, **env)
    assert f"over {parts} device part(s)" in line
    if kind == "asan" and not devices:
        # the switches reach code that allocates: the run passes more allocation fault points than one with them off (at least what
        # tests/test_temporal_sanitizers.py asks of the temporal switch alone)
        assert _fault_points(_run(soaks[kind], 2, **ON)) > _fault_points(_run(soaks[kind], 2)) + 10


@pytest.mark.parametrize("devices", ["", "0,1"])
def test_failed_allocations_with_both_switches_on(soaks, devices):
    """A spread of failed allocations over the run: the call that is hit returns nothing, everything after it works, the pool ends empty."""
    env = dict(ON)
    if devices:
        env["LSN_HOST_DEVICES"] = devices
    for n in (5, 12, 19, 26, 40, 75, 150, 300, 500):
        _run(soaks["asan"], 2, LSN_TEST_FAIL_ALLOC=str(n), **env)
