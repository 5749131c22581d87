"""What the fifteen entry points that take witness or selector columns answer to a bad call: run_cases(ctx) maps a case name
to [return code, typlonk_last_error text] ("" where the call was accepted).  tests/golden/column_refusals.json holds these
answers as the parent of the column carrier gave them (tools/record_column_refusals.py); tests/test_gpu_column_refusals.py
compares.  Only the C ABI is used, so the module runs against any build of the library.

The shape: the squaring chain at log_n = 3, an SRS of n + 3 points and one of n - 1, two witnesses per batched call, every
public value 0 (so the chain's own columns satisfy the circuit under any pi_len).  A case is one mistake, or two mistakes
that one call can carry (the pairs pin which refusal wins); then count == 0 with everything null; then one good call per
entry point, recorded as the SHA-256 of what it wrote."""
import ctypes as C
import hashlib
from itertools import combinations

import numpy as np

from typlonk_amd import capi
from typlonk_amd.circuits import SquaringChain

LOG_N = 3
N = 1 << LOG_N
SIZE_MAX = C.c_size_t(-1).value
U64P = C.POINTER(C.c_uint64)
U32P = C.POINTER(C.c_uint32)
PI_LEN = (2, 3)      # the good call's pi_len of witness 0 and 1 (the compact rule)
CAP = 4              # typlonk_witness_check's list capacity
UNKNOWN_ID = 99999


class Entry:
    def __init__(self, name, form, k=3, count=1, pi=None, rows=False, sid=True, cid=True, busy=True, batched=False):
        self.name, self.form, self.k, self.count, self.pi = name, form, k, count, pi
        self.rows, self.sid, self.cid, self.busy, self.batched = rows and form == "host", sid, cid, busy, batched


def _both(name, **kw):
    return [Entry(name, "dev", **kw), Entry(name + "_host", "host", **kw)]


ENTRIES = ([Entry("typlonk_prover_round1", "dev", pi="ref")]
           + _both("typlonk_prove", pi="ref")
           + _both("typlonk_prove_compact", pi="compact", rows=True)
           + _both("typlonk_prove_batch", pi="ref", count=2, batched=True)
           + _both("typlonk_prove_batch_compact", pi="compact", rows=True, count=2, batched=True)
           + _both("typlonk_witness_check", pi="compact", rows=True, count=2, batched=True, sid=False, busy=False)
           + _both("typlonk_circuit_compile", k=5, rows=True, sid=False, cid=False, busy=False)
           + _both("typlonk_circuit_compile_pairs", k=5, rows=True, sid=False, cid=False, busy=False))


def good_state(e):
    return {"cols": ["ok"] * (e.k * e.count), "cols_null": False, "rows": N, "pi": ["ok"] * e.count, "pi_null": False,
            "len": list(PI_LEN[:e.count]), "len_null": False, "cid": "ok", "sid": "ok", "busy": False}


def mistakes(e):
    """[(name, the slots of the call it occupies, what it does to a state)]: two mistakes fit into one call when their slots
    are disjoint"""
    K = e.k * e.count
    out = []

    def add(name, slots, **change):
        def apply(st):
            for key, (at, val) in change.items():
                if at is None:
                    st[key] = val
                else:
                    st[key][at] = val
        out.append((name, frozenset(slots), apply))

    add("cols=NULL", [f"col{i}" for i in range(K)], cols_null=(None, True))
    for i in sorted({0, K // 2, K - 1}):          # first, middle, last (a batch: the last column of the second witness)
        add(f"col[{i}]=NULL", [f"col{i}"], cols=(i, "null"))
        if e.form == "dev":
            add(f"col[{i}]:n-1", [f"col{i}"], cols=(i, "short"))
    if e.rows:
        for tag, v in (("0", 0), ("n-1", N - 1), ("n+1", N + 1), ("SIZE_MAX", SIZE_MAX)):
            add(f"rows={tag}", ["rows"], rows=(None, v))
    if e.pi == "compact":
        if e.batched:
            add("pi=NULL", [f"pi{j}" for j in range(e.count)], pi_null=(None, True))
            add("pi_len=NULL", [f"len{j}" for j in range(e.count)], len_null=(None, True))
        for j in range(e.count):
            add(f"pi_len[{j}]=n+1", [f"len{j}"], len=(j, N + 1))
            add(f"pi[{j}]=NULL", [f"pi{j}"], pi=(j, "null"))
            if e.form == "dev":
                add(f"pi[{j}]:pi_len-1", [f"pi{j}"], pi=(j, "short"))
    if e.pi == "ref" and e.form == "dev":
        for j in range(e.count):
            add(f"pi[{j}]:n-1", [f"pi{j}"], pi=(j, "short"))
    if e.cid:
        add("circuit=unknown", ["cid"], cid=(None, "unknown"))
    if e.sid:
        add("srs=unknown", ["sid"], sid=(None, "unknown"))
        add("srs:n-1", ["sid"], sid=(None, "short"))
    if e.busy:
        add("prover_busy", ["busy"], busy=(None, True))
    return out


class Env:
    """the circuit, the two SRS and every column a case may pass, made once"""

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib
        self.chain = SquaringChain(ctx, LOG_N, keep_host=True)
        host = self.chain.host_inputs()
        self.cid = self.chain.circuit
        self.ks = capi._cosets_arg(self.chain.cosets)
        secret = np.array([0x5EC2E7D00D51, 0, 0, 0], dtype=np.uint64)
        self.sid = ctx.srs_generate(secret, N + 3)
        self.sid_short = ctx.srs_generate(secret, N - 1)
        self.wire_bufs = list(self.chain.wire_evals)
        self.wire_host = [np.ascontiguousarray(w) for w in host["wires"]]
        self.sel_host = [np.ascontiguousarray(s) for s in host["selectors"]]
        self.sel_bufs = []
        for s in self.sel_host:
            b = ctx.alloc(N)
            b.upload(s)
            self.sel_bufs.append(b)
        self.pi_host = np.zeros((N + 2, 4), dtype=np.uint64)
        self._zeros = {}
        self.short = self.zeros(N - 1)
        self.pairs = np.array([[0, N]], dtype=np.uint32)       # a_0 = b_0

    def zeros(self, size):
        """a device buffer of exactly `size` zero elements"""
        if size not in self._zeros:
            b = self.ctx.alloc(size)
            b.upload(np.zeros((size, 4), dtype=np.uint64))
            self._zeros[size] = b
        return self._zeros[size]

    def free(self):
        for b in self.sel_bufs + list(self._zeros.values()):
            b.free()
        self.ctx.srs_free(self.sid)
        self.ctx.srs_free(self.sid_short)
        self.chain.free()

    def last_error(self):
        return self.lib.typlonk_last_error(self.ctx.h).decode()


def call(env, e, st):
    """the raw call of entry point `e` that `st` describes: (return code, the bytes it wrote)"""
    lib, h, dev = env.lib, env.ctx.h, e.form == "dev"
    K = e.k * e.count
    if st["cols_null"]:
        cols = None
    elif dev:
        src = env.sel_bufs if e.k == 5 else env.wire_bufs * e.count
        cols = (C.c_void_p * K)(*[None if c == "null" else (env.short if c == "short" else src[i]).handle.value
                                  for i, c in enumerate(st["cols"])])
    else:
        src = env.sel_host if e.k == 5 else env.wire_host * e.count
        cols = (U64P * K)(*[None if c == "null" else capi._u64p(src[i]) for i, c in enumerate(st["cols"])])

    def pi_item(j):
        p = st["pi"][j]
        if p == "null":
            return None
        if not dev:
            return capi._u64p(env.pi_host)
        size = N if e.pi == "ref" else st["len"][j]
        return env.zeros(size - 1 if p == "short" else size).handle.value

    if e.pi and e.batched:
        pis = None if st["pi_null"] else ((C.c_void_p if dev else U64P) * e.count)(*[pi_item(j) for j in range(e.count)])
        lens = None if st["len_null"] else (C.c_size_t * e.count)(*st["len"])
    elif e.pi:
        pi0, len0 = pi_item(0), st["len"][0]
    cid = env.cid if st["cid"] == "ok" else UNKNOWN_ID
    sid = {"ok": env.sid, "unknown": UNKNOWN_ID, "short": env.sid_short}[st["sid"]]
    rows, ks = st["rows"], C.byref(env.ks)
    fn = getattr(lib, e.name)
    base = e.name[:-5] if e.form == "host" else e.name

    if base == "typlonk_prover_round1":
        pr, cxy, cinf = C.c_void_p(), ((C.c_uint64 * 12) * 3)(), (C.c_uint8 * 3)()
        rc = fn(h, sid, cid, cols, pi0, C.byref(pr), C.byref(cxy), C.byref(cinf))
        if pr.value:
            lib.typlonk_prover_free(pr)
        return rc, bytes(cxy) + bytes(cinf)
    if base == "typlonk_prove":
        out = capi.Proof()
        return fn(h, sid, cid, cols, pi0, ks, C.byref(out)), bytes(out)
    if base == "typlonk_prove_compact":
        out = capi.ProofCompact()
        args = (cols, pi0, len0) if dev else (cols, rows, pi0, len0)
        return fn(h, sid, cid, *args, ks, C.byref(out)), bytes(out)
    if base == "typlonk_prove_batch":
        out, status = (capi.Proof * e.count)(), (C.c_int * e.count)()
        return fn(h, sid, cid, cols, pis, e.count, ks, out, status), bytes(out) + bytes(status)
    if base == "typlonk_prove_batch_compact":
        out, status = (capi.ProofCompact * e.count)(), (C.c_int * e.count)()
        args = (cols, pis, lens) if dev else (cols, rows, pis, lens)
        return fn(h, sid, cid, *args, e.count, ks, out, status), bytes(out) + bytes(status)
    if base == "typlonk_witness_check":
        reports = (capi.WitnessReport * e.count)()
        gate, copy = (C.c_uint32 * (e.count * CAP))(), (C.c_uint32 * (2 * e.count * CAP))()
        args = (cols, pis, lens) if dev else (cols, rows, pis, lens)
        return fn(h, cid, *args, e.count, ks, CAP, reports, gate, copy), bytes(reports) + bytes(gate) + bytes(copy)
    # the four compiles: what the call made is told by the circuit's commitments, then the circuit is freed again
    new_id, info = C.c_uint32(), C.c_uint64()
    perm = (env.pairs.ctypes.data_as(U32P), env.pairs.shape[0]) if base == "typlonk_circuit_compile_pairs" else (None,)
    args = (cols, *perm) if dev else (cols, rows, *perm)
    rc = fn(h, *args, ks, LOG_N, C.byref(new_id), C.byref(info))
    wrote = b""
    if rc == 0:
        for xy, inf in env.ctx.circuit_commitments(env.sid, new_id.value):
            wrote += xy.tobytes() + bytes([inf])
        wrote += bytes(info)
        env.ctx.circuit_free(new_id.value)
    return rc, wrote


def _cases(e):
    """[(case name, state)] of one entry point: every mistake, every pair that fits into one call"""
    ms = mistakes(e)
    groups = [(m,) for m in ms] + [p for p in combinations(ms, 2) if not (p[0][1] & p[1][1])]
    out = []
    for g in groups:
        st = good_state(e)
        for _, _, apply in g:
            apply(st)
        out.append((e.name + ": " + " + ".join(m[0] for m in g), st))
    return out


def _null_count_zero(env, e):
    lib, h, dev = env.lib, env.ctx.h, e.form == "dev"
    fn = getattr(lib, e.name)
    rows = () if dev else (N,)
    if "witness_check" in e.name:
        return fn(h, env.cid, None, *rows, None, None, 0, None, CAP, None, None, None)
    if "compact" in e.name:
        return fn(h, env.sid, env.cid, None, *rows, None, None, 0, None, None, None)
    return fn(h, env.sid, env.cid, None, None, 0, None, None, None)


def run_cases(ctx):
    env = Env(ctx)
    got = {}

    def record(name, e, st):
        rc, _ = call(env, e, st)
        got[name] = [rc, env.last_error() if rc else ""]

    try:
        every = [(e, name, st) for e in ENTRIES for name, st in _cases(e)]
        for e, name, st in every:
            if not st["busy"]:
                record(name, e, st)
        # the cases with a round-by-round prover open on the context
        pr, cxy, cinf = C.c_void_p(), ((C.c_uint64 * 12) * 3)(), (C.c_uint8 * 3)()
        w3 = (C.c_void_p * 3)(*[b.handle.value for b in env.wire_bufs])
        rc = env.lib.typlonk_prover_round1(ctx.h, env.sid, env.cid, w3, None, C.byref(pr), C.byref(cxy), C.byref(cinf))
        if rc:
            raise RuntimeError("typlonk_prover_round1 refused the good call: " + env.last_error())
        try:
            for e, name, st in every:
                if st["busy"]:
                    record(name, e, st)
        finally:
            env.lib.typlonk_prover_free(pr)
        for e in ENTRIES:
            if e.batched:
                got[e.name + ": count=0, everything NULL"] = [_null_count_zero(env, e), ""]
        # the context is still usable: one good call per entry point
        for e in ENTRIES:
            rc, wrote = call(env, e, good_state(e))
            got[e.name + ": good call"] = [rc, hashlib.sha256(wrote).hexdigest()]
    finally:
        env.free()
    return got
