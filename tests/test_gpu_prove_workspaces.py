"""The provers' workspaces (csrc/prove_plan.hpp: prover_mem, ops_tmp, quot_ext, quot_tab, batch_tab, the pinned slots) on ONE
context shared by calls of different size and shape, so that every workspace is first sized by a small user and then grown by
a larger one -- what no other test does: each of them proves one size per context.  Every result must equal, word for word,
the same call made on a fresh context of its own.  The sizes are the smallest at which a wrong offset, a short carry run or a
stale pointer after a re-allocation shows: 2^3 (n = 8: round 2 of a proof asks ops_tmp for 41 elements, round 3 for 16384) and
2^12 (n = 4096, two scan blocks, so carries are indexed past the first block)."""
import numpy as np
import pytest

import typlonk_amd
from helpers import O
from test_gpu_prove_batch import Circuit, single

pytestmark = pytest.mark.gpu

SMALL, LARGE = 3, 12


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % O.R), dtype=np.uint64)


def words(x):
    """every word of a result, in order: dicts by key, lists and tuples by position"""
    if isinstance(x, dict):
        return b"".join(words(x[k]) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return b"".join(words(v) for v in x)
    return np.ascontiguousarray(x, dtype=np.uint64).tobytes()


def residues(seed, n):
    """n field elements as (n, 4) limbs (any residue below 2^254 will do: the calls here are exact on all of them)"""
    return np.random.default_rng(seed).integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)


class Env:
    """a context's circuits and witnesses, built on first use"""

    def __init__(self, ctx):
        self.ctx, self.circuits, self.held = ctx, {}, []

    def circuit(self, log_n):
        if log_n not in self.circuits:
            self.circuits[log_n] = Circuit(self.ctx, log_n)
        return self.circuits[log_n]

    def buf(self, arr):
        b = self.ctx.alloc(len(arr))
        b.upload(arr)
        self.held.append(b)
        return b

    def witnesses(self, log_n, ks):
        c = self.circuit(log_n)
        bufs, pibs = c.upload([c.witness(k, pi=(k % 2 == 1)) for k in ks])
        self.held += [b for bs in bufs for b in bs] + [b for b in pibs if b is not None]
        return c, bufs, pibs

    def free(self):
        for b in self.held:
            b.free()
        for c in self.circuits.values():
            c.free()


def open_small(e):
    q = e.ctx.alloc(8)
    e.held.append(q)
    y = e.ctx.open_dev(e.buf(residues(1, 8)), 8, _limbs(0xABCDEF), q)
    return [y, q.download(0, 7)]


def grand_product_small(e):
    c, bufs, _ = e.witnesses(SMALL, [0])
    sigma = [e.buf(s) for s in c.chain.host_inputs()["sigma"]]
    z = e.ctx.alloc(c.n)
    e.held.append(z)
    e.ctx.grand_product_dev(SMALL, bufs[0], sigma, _limbs(0x1234567), _limbs(0x7654321), c.cosets, z)
    return z.download()


def prove_at(log_n, k):
    def step(e):
        c, bufs, pibs = e.witnesses(log_n, [k])
        return e.ctx.prove_native(c.sid, c.cid, bufs[0], pibs[0], c.cosets)
    return step


def prove_batch_at(log_n, count):
    def step(e):
        c, bufs, pibs = e.witnesses(log_n, range(count))
        return list(e.ctx.prove_batch(c.sid, c.cid, bufs, pibs, c.cosets))
    return step


def prove_compact_large(e):
    c, bufs, pibs = e.witnesses(LARGE, [1])
    return e.ctx.prove_compact(c.sid, c.cid, bufs[0], pibs[0], c.n - 3, c.cosets)


def prove_batch_compact_small(e):
    c, bufs, pibs = e.witnesses(SMALL, range(5))
    return list(e.ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, [c.n - 3 if p is not None else 0 for p in pibs], c.cosets))


def quotient_large_uncached(e):
    n = 1 << LARGE
    b = [e.buf(residues(100 + i, n)) for i in range(13)]
    t = e.ctx.alloc(4 * n)
    e.held.append(t)
    e.ctx.quotient_dev(LARGE, b[0:3], b[3], b[4:9], b[9:12], b[12], _limbs(5), _limbs(6), _limbs(7), [_limbs(k) for k in (2, 3, 4)], t)
    return t.download()


def prove_rounds_batched_large(e):
    c, bufs, pibs = e.witnesses(LARGE, [2])
    d = e.ctx.prove(c.sid, c.cid, bufs[0], pibs[0], c.cosets, challenge_v=lambda evals: _limbs(0xF00D))
    return {k: v for k, v in d.items() if k != "batched"}


STEPS = [open_small, grand_product_small, prove_at(SMALL, 0), prove_batch_at(LARGE, 3), prove_compact_large,
         prove_batch_compact_small, quotient_large_uncached, prove_rounds_batched_large, prove_at(SMALL, 0)]


def on_fresh_context(step):
    ctx = typlonk_amd.Context(0)
    e = Env(ctx)
    try:
        return words(step(e))
    finally:
        e.free()
        ctx.close()


def test_calls_of_mixed_size_and_shape_on_one_context_equal_each_call_on_a_fresh_one(built):
    ctx = typlonk_amd.Context(0)
    shared = Env(ctx)
    try:
        got = [words(step(shared)) for step in STEPS]
    finally:
        shared.free()
        ctx.close()
    assert got[2] == got[8] and len(got[2]) > 0
    for i, step in enumerate(STEPS):
        assert got[i] == on_fresh_context(step), i


def test_two_waves_of_small_proofs_after_a_large_batch_equal_single_proofs(built):
    """65 proofs at 2^3 are two waves, of 64 and of 1, in an arena and slots a 2^12 batch of 3 has sized"""
    ctx = typlonk_amd.Context(0)
    shared = Env(ctx)
    try:
        prove_batch_at(LARGE, 3)(shared)
        proofs, st = prove_batch_at(SMALL, 65)(shared)
    finally:
        shared.free()
        ctx.close()
    ctx = typlonk_amd.Context(0)
    e = Env(ctx)
    try:
        c, bufs, pibs = e.witnesses(SMALL, range(65))
        for k in range(65):
            rc, ref = single(ctx, c.sid, c.cid, bufs[k], pibs[k], c.cosets)
            assert (st[k], words(proofs[k])) == (rc, words(ref)), k
    finally:
        e.free()
        ctx.close()
