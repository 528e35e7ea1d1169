"""An independent numpy float32 restatement of include/rtr_accum.h — what rtr_accumulate_paths adds to an image and the throughput it
hands on, and what rtr_gather_records gathers — with the synthetic records the host and GPU tests run it on.

The witness works on whole arrays, one numpy float32 operation per step of the rule (numpy's float32 multiply and add are single
IEEE-754 binary32 operations), and shares no code with the library.  The inputs hold no NaN, whose payloads no rule fixes."""
import ctypes as C

import numpy as np

SURFACE_MISS, SURFACE_OBJECT, SURFACE_LIGHT, SURFACE_INVALID = 0, 1, 2, 3
LIGHTS_FROM_EMITTERS, MISSES_FROM_ESCAPES = 1, 2
PATH_NONE = 0xffffffff
GUARD_WORDS = 8
GUARD = 0xA5A5A5A5


def witness_accumulate(radiance, T, ids, emitters, escapes, sky, bounces, flags, num_slots, accum, out_term):
    """radiance (N, 12), emitters, escapes, bounces (N, 8) uint32 words or None; T (N, 3), sky (N, 4) float32 or None; ids (N,) uint32
    or None; accum, out_term (S, 3) float32 (out_term or None) -> (accum, out_term, out_throughput), new arrays"""
    n = radiance.shape[0]
    kind = radiance[:, 3]
    rad = radiance[:, 0:3].copy().view(np.float32)
    zeros = np.zeros((n, 3), np.float32)
    if flags & LIGHTS_FROM_EMITTERS:
        rad = np.where((kind == SURFACE_LIGHT)[:, None], emitters[:, 0:3].copy().view(np.float32) if emitters is not None else zeros, rad)
    if flags & MISSES_FROM_ESCAPES:
        rad = np.where((kind == SURFACE_MISS)[:, None], escapes[:, 0:3].copy().view(np.float32) if escapes is not None else zeros, rad)
    T = T.astype(np.float32, copy=True)
    term = np.multiply(T, rad, dtype=np.float32)
    if sky is not None:
        term = np.add(term, np.multiply(T, sky[:, 0:3], dtype=np.float32), dtype=np.float32)
    slot = np.arange(n, dtype=np.uint32) if ids is None else ids.astype(np.uint32)
    ok = slot < np.uint32(num_slots)
    assert len(set(slot[ok].tolist())) == int(ok.sum()), "the witness needs distinct ids"
    accum = accum.copy()
    accum[slot[ok]] = np.add(accum[slot[ok]], term[ok], dtype=np.float32)
    if out_term is not None:
        out_term = out_term.copy()
        out_term[slot[ok]] = term[ok]
    out_t = np.multiply(T, bounces[:, 0:3].copy().view(np.float32), dtype=np.float32) if bounces is not None else None
    return accum, out_term, out_t


def witness_gather(src, rows):
    """numpy.take with zero rows for the indices that are not rows of src"""
    rows = rows.astype(np.uint32)
    ok = rows < np.uint32(src.shape[0])
    out = np.zeros((rows.shape[0],) + src.shape[1:], src.dtype)
    if ok.any():
        out[ok] = np.take(src, rows[ok].astype(np.int64), axis=0)
    return out


# ---- synthetic records -------------------------------------------------------------------------------------------------------------
def guarded(words):
    """a 16-B aligned uint32 buffer: GUARD_WORDS guard words, the payload, GUARD_WORDS guard words -> (buffer, payload view)"""
    words = np.ascontiguousarray(words).view(np.uint32).reshape(-1)
    raw = np.empty(words.size + 2 * GUARD_WORDS + 4, np.uint32)
    off = ((-raw.ctypes.data) % 16) // 4
    buf = raw[off:off + words.size + 2 * GUARD_WORDS]
    buf[:] = GUARD
    buf[GUARD_WORDS:GUARD_WORDS + words.size] = words
    return buf, buf[GUARD_WORDS:GUARD_WORDS + words.size]


def guards_intact(buf):
    return bool((buf[:GUARD_WORDS] == GUARD).all() and (buf[-GUARD_WORDS:] == GUARD).all())


def _floats(rng, shape):
    """finite float32 values of both signs with zeros, a negative zero and some tiny ones (whose products are subnormal) mixed in"""
    x = rng.uniform(-1.0, 2.0, shape).astype(np.float32)
    pick = rng.integers(0, 16, shape)
    x[pick == 0] = 0.0
    x[pick == 1] = -0.0
    x[pick == 2] = np.float32(1e-22)
    return x


class AccumCase:
    """One call's arrays.  ids: "identity" (pathIds NULL), "permutation", or "mixed" (a permutation with RTR_PATH_NONE, numSlots and
    numSlots + 5 put in).  t_words, image_words: the strides in words.  inplace: outThroughput is the input throughput (t_words 3)."""

    def __init__(self, n, num_slots=None, ids="identity", flags=0, emitters=False, escapes=False, sky=False, bounces=False, term=False, t_words=3,
                 image_words=3, inplace=False, seed=1):
        rng = np.random.default_rng(seed + 1000 * n)
        self.n, self.flags, self.t_words, self.image_words, self.inplace = n, flags, t_words, image_words, inplace
        self.num_slots = S = n if num_slots is None else num_slots
        rad = rng.integers(0, 2 ** 32, (n, 12), dtype=np.uint32)          # the words the rule does not read are noise
        rad[:, 0:3] = _floats(rng, (n, 3)).view(np.uint32)
        rad[:, 3] = np.arange(n, dtype=np.uint32) % 4 if n < 16 else rng.integers(0, 4, n, dtype=np.uint32)
        self.radiance = rad
        self.T = rng.integers(0, 2 ** 32, (n, t_words), dtype=np.uint32)
        self.T[:, 0:3] = np.abs(_floats(rng, (n, 3))).view(np.uint32)
        kind = rad[:, 3]

        def records(counts_where, kind_word):
            rec = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint32)     # rows that do not count hold noise: the rule must not read them
            rec[:, 0:3] = _floats(rng, (n, 3)).view(np.uint32)
            rec[counts_where, 0:3] = rng.uniform(0.25, 3.0, (int(counts_where.sum()), 3)).astype(np.float32).view(np.uint32)
            rec[counts_where, 7] = kind_word
            return rec
        self.emitters = records(kind == SURFACE_LIGHT, SURFACE_LIGHT) if emitters else None
        self.escapes = records(kind == SURFACE_MISS, SURFACE_MISS) if escapes else None
        self.bounces = records(np.zeros(n, bool), 0) if bounces else None
        self.sky = _floats(rng, (n, 4)) if sky else None
        if ids == "identity":
            self.ids = None
        else:
            self.ids = rng.permutation(max(n, S)).astype(np.uint32)[:n]
            if ids == "mixed" and n >= 4:
                at = rng.choice(n, min(n, max(3, n // 5)), replace=False)
                self.ids[at] = np.resize(np.array([PATH_NONE, S, S + 5], np.uint32), at.size)
        self.accum0 = np.zeros((S, image_words), np.float32)
        self.accum0[:, 0:3] = _floats(rng, (S, 3))
        self.accum0[:, 3:] = 7.0
        self.term0 = np.full((S, image_words), 9.0, np.float32) if term else None

    def slots(self):
        return np.arange(self.n, dtype=np.uint32) if self.ids is None else self.ids

    def params(self, A):
        return A.rtr_accum_params(self.flags, self.num_slots, 4 * self.t_words, 4 * self.image_words, (A.u32 * 4)(0, 0, 0, 0))

    def expected(self):
        """(accum, out_term, out_throughput) as the witness has them, in the call's own layouts"""
        T = np.ascontiguousarray(self.T[:, 0:3]).view(np.float32)
        acc, term, out_t = witness_accumulate(self.radiance, T, self.ids, self.emitters, self.escapes, self.sky, self.bounces, self.flags, self.num_slots,
                                              np.ascontiguousarray(self.accum0[:, 0:3]), None if self.term0 is None else np.ascontiguousarray(self.term0[:, 0:3]))
        full_acc = self.accum0.copy()
        full_acc[:, 0:3] = acc
        full_term = None
        if term is not None:
            full_term = self.term0.copy()
            full_term[:, 0:3] = term
        return full_acc, full_term, out_t

    def host_buffers(self):
        """name -> (guarded buffer, payload view) of every array of the call; absent arrays map to None"""
        out = {}
        for name, x in (("radiance", self.radiance), ("T", self.T), ("ids", self.ids), ("emitters", self.emitters), ("escapes", self.escapes), ("sky", self.sky),
                        ("bounces", self.bounces), ("accum", self.accum0), ("term", self.term0)):
            out[name] = guarded(x) if x is not None else None
        out["out_t"] = None
        if self.bounces is not None and not self.inplace:
            out["out_t"] = guarded(np.full((self.n, 3), 5.0, np.float32))
        return out


def call_accumulate(fn, handle, case, A, address):
    """fn: rtr_host_accumulate_paths (handle None) or a device entry point (handle: the context's); address: name -> the payload's
    address or None.  -> the status"""
    def vp(name):
        a = address(name) if case.n else None
        return C.c_void_p(a) if a else None
    p = case.params(A)
    out_t = vp("T") if case.inplace else vp("out_t")
    args = (vp("radiance"), vp("T"), vp("ids"), vp("emitters"), vp("escapes"), vp("sky"), vp("bounces"), case.n, C.byref(p), vp("accum"), vp("term"), out_t)
    return fn(*args) if handle is None else fn(handle, *args)


def optional_cases(n, seed=3):
    """the optional-array, flag, stride and id combinations the host and the GPU tests share, at n paths"""
    both = LIGHTS_FROM_EMITTERS | MISSES_FROM_ESCAPES
    cases = []
    for flags in (0, LIGHTS_FROM_EMITTERS, MISSES_FROM_ESCAPES, both):
        for present in (False, True):
            cases.append(AccumCase(n, flags=flags, emitters=present, escapes=present, sky=present, bounces=present, term=present, ids="mixed" if present else "identity",
                                   seed=seed + len(cases)))
    for e, s, k, b, t in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 0, 1, 0, 1), (0, 1, 0, 1, 0)):
        cases.append(AccumCase(n, flags=both, emitters=bool(e), escapes=bool(s), sky=bool(k), bounces=bool(b), term=bool(t), ids="permutation", seed=seed + len(cases)))
    for t_words in (3, 4, 8):
        for image_words in (3, 4):
            cases.append(AccumCase(n, flags=both, emitters=True, escapes=True, sky=True, bounces=True, term=True, ids="mixed", t_words=t_words,
                                   image_words=image_words, seed=seed + len(cases)))
    for ids in ("identity", "permutation", "mixed"):
        for num_slots in (n, n + 9, max(1, n - 7)):
            cases.append(AccumCase(n, num_slots=num_slots, ids=ids, flags=both, emitters=True, escapes=True, sky=True, bounces=True, term=True, seed=seed + len(cases)))
    cases.append(AccumCase(n, flags=both, emitters=True, escapes=True, sky=True, bounces=True, term=True, ids="mixed", inplace=True, seed=seed + len(cases)))
    return cases
