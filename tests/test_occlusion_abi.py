"""The queued occlusion query's C-ABI surface (rtr_occlusion_scratch_bytes, rtr_trace_occlusion[_async]) — what needs no device: the
header declares the entry points, the product and the test library export them, _abi.py binds them, the ABI version stays 3, the
scratch size is pure arithmetic (monotone, 16-B granular), and the argument errors that come before any device work."""
import ctypes as C
import os
import re
import subprocess

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rtr_occlusion_scratch_bytes", "rtr_trace_occlusion_async", "rtr_trace_occlusion")
INVALID = -1


def _bytes(lib, n):
    b = C.c_size_t(0)
    assert lib.rtr_occlusion_scratch_bytes(n, C.byref(b)) == 0
    return int(b.value)


def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtr_[a-z0-9_]+)\s*\(", text))
    for path in (A.LIB_HIP_PATH, A.LIB_HIP_HOOKS_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        for n in NAMES:
            assert n in declared, f"{n} is not declared in include/rtr.h"
            assert n in exported, f"{os.path.basename(path)} does not export {n}"
            assert n in A.RTR_SYMBOLS, f"{n} is not bound in _abi.RTR_SYMBOLS"
    assert A.hip_lib().rtr_abi_version() == 3
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+3\b", open(os.path.join(ROOT, "include", "rtr.h")).read())
    assert callable(api.trace_occlusion)


def test_scratch_bytes_is_pure_arithmetic():
    lib = A.hip_lib()                       # no context, no device
    assert lib.rtr_occlusion_scratch_bytes(100, None) == INVALID
    assert b"null" in lib.rtr_last_error()
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 1 << 20, (1 << 20) + 1, 26956800, (100 << 20) - 1, 100 << 20,
             (100 << 20) + 1, 1 << 31, 0xffffffff]
    last = _bytes(lib, 0)
    assert last % 16 == 0
    for n in sizes:
        b = _bytes(lib, n)
        assert b % 16 == 0, n
        assert b >= last, f"not monotone at {n}"
        assert b >= 4 * n, "the queue holds one index per ray"
        last = b
    assert _bytes(lib, 26956800) < 5 * 26956800, "indices, not rays: about 4 B per ray on a long array"
    assert api.occlusion_scratch_bytes(lib, 4096) == _bytes(lib, 4096)


def test_argument_errors_that_need_no_device():
    lib = A.hip_lib()
    fake = A.VP(0x1000)
    assert lib.rtr_trace_occlusion(None, None, fake, 64, 0, fake, 1 << 20, fake, None) == INVALID
    assert b"null context or scene" in lib.rtr_last_error()
    assert lib.rtr_trace_occlusion_async(None, None, fake, 64, 0, fake, 1 << 20, fake) == INVALID
    assert b"rtr_trace_occlusion_async" in lib.rtr_last_error()
