"""ctypes binding of the numerical-contract probe (tests/math_probe/): the op table of math_ops.h compiled by the oracle's compile
line (libmath_probe_host.so) and by the product's (libmath_probe.so, gfx950).  TEST INFRASTRUCTURE: nothing under
realtimeraytracer_amd/ refers to it."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
HOST_PATH = os.path.join(_HERE, "math_probe", "libmath_probe_host.so")
DEVICE_PATH = os.path.join(_HERE, "math_probe", "libmath_probe.so")
CHUNK = 1 << 20                     # PROBE_CHUNK_LOG2: patterns per digest
QNAN = np.uint32(0x7FC00000)


class Probe:
    def __init__(self, path, make_dir, target):
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", os.path.join(_ROOT, make_dir), target], stdout=subprocess.DEVNULL)
        L = self.lib = C.CDLL(path)
        L.math_probe_op_name.restype = C.c_char_p
        L.math_probe_op_fmask.restype = C.c_uint32
        L.math_probe_eval.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        L.math_probe_sweep.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]
        self.names = [L.math_probe_op_name(i).decode() for i in range(L.math_probe_op_count())]
        self.index = {n: i for i, n in enumerate(self.names)}
        self.nin = {n: L.math_probe_op_nin(i) for i, n in enumerate(self.names)}
        self.nout = {n: L.math_probe_op_nout(i) for i, n in enumerate(self.names)}
        self.fmask = {n: L.math_probe_op_fmask(i) for i, n in enumerate(self.names)}

    def eval(self, op, words):
        """words: (n, nin) uint32 (or float32, taken as bit patterns) -> (n, nout) uint32"""
        a = np.ascontiguousarray(words)
        if a.dtype == np.float32:
            a = a.view(np.uint32)
        assert a.dtype == np.uint32
        a = a.reshape(-1, self.nin[op])
        out = np.empty((a.shape[0], self.nout[op]), np.uint32)
        rc = self.lib.math_probe_eval(0, self.index[op], a.ctypes.data, a.shape[0], out.ctypes.data)
        if rc:
            raise RuntimeError(f"math_probe_eval({op}) failed: {rc}")
        return out

    def sweep(self, op, first, count, stride=1):
        """digests of the patterns first + i * stride (mod 2^32), i < count: one uint64 per 2^20 consecutive i"""
        out = np.zeros((count + CHUNK - 1) // CHUNK, np.uint64)
        rc = self.lib.math_probe_sweep(0, self.index[op], first & 0xFFFFFFFF, count, stride, out.ctypes.data)
        if rc:
            raise RuntimeError(f"math_probe_sweep({op}) failed: {rc}")
        return out


_host = _device = None


def host():
    global _host
    if _host is None:
        _host = Probe(HOST_PATH, "oracle", "../tests/math_probe/libmath_probe_host.so")
    return _host


def device():
    """loading needs no GPU; eval and sweep do"""
    global _device
    if _device is None:
        _device = Probe(DEVICE_PATH, os.path.join("realtimeraytracer_amd", "csrc"), "../../tests/math_probe/libmath_probe.so")
    return _device


def canon(op, probe, out):
    """the comparison rule's NaN clause: every NaN in a float output becomes one pattern"""
    out = out.copy()
    for k in range(out.shape[1]):
        if (probe.fmask[op] >> k) & 1:
            col = out[:, k]
            col[(col & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = QNAN
    return out


def zeros_by_value(op, probe, out):
    """for the ops whose zero sign is not part of the contract (rtr_hwmin / rtr_hwmax and what is built on them, rtr_div_by)"""
    out = out.copy()
    for k in range(out.shape[1]):
        if (probe.fmask[op] >> k) & 1:
            col = out[:, k]
            col[col == np.uint32(0x80000000)] = 0
    return out
