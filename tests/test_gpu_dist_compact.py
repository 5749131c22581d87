"""The compact proof shape on a sharded SRS, folded across the ranks (include/typlonk.h, "The compact shape on a shard").
RCCL refuses two ranks per device, so the ranks are fresh processes on GPU 0 (tests/dist_compact_worker.py) whose all-gather is
carried by the test-only tests/cpp/libfake_rccl.so; the staging, the fixed record schedule (12, 1, 3, 2), the rank-order fold
and the failure protocol are the product's code.  Every comparison with the whole-SRS result is exact equality of bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu


def _ranks(world, log_n, tmp_path, steps, tables=False, srs="generate", pi_lens="0,1,n", timeout=900, prepare=None):
    """start `world` fresh rank processes of tests/dist_compact_worker.py on GPU 0 over the stand-in exchange library; every
    rank has a timeout, and all are killed when one runs into it"""
    from test_gpu_compact import _g2s

    assert world <= 8
    fake = os.path.join(ROOT, "tests", "cpp", "libfake_rccl.so")
    assert os.path.exists(fake), "tests/cpp/libfake_rccl.so not built (__graft_entry__.build())"
    np.save(os.path.join(str(tmp_path), "g2s.npy"), _g2s())
    if prepare:
        prepare()
    procs = []
    for r in range(world):
        env = dict(os.environ, TYPLONK_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_S="300", TABLES="1" if tables else "0", SRS=srs,
                   STEPS=",".join(steps), PI_LENS=pi_lens)
        env.pop("TYPLONK_TEST_COMM_FAIL_STAGING", None)
        if "staging" in steps and r == world - 1:
            # this rank's FIRST fold loses its staging copy: the fault injection exists only in the test build of the
            # library (-DTYPLONK_TEST_HOOKS); every other rank runs the shipped one
            hooked = os.path.join(ROOT, "tests", "cpp", "hooks", "libtyplonk_hip.so")
            assert os.path.exists(hooked), "tests/cpp/hooks/libtyplonk_hip.so not built (__graft_entry__.build())"
            env["TYPLONK_LIB_PATH"] = hooked
            env["TYPLONK_TEST_COMM_FAIL_STAGING"] = "1"
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_compact_worker.py"), str(r), str(world),
                                       str(tmp_path), str(log_n)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True, cwd=ROOT))
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            outs.append(o)
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
                q.wait()
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-1500:] for o in outs)
    return [json.load(open(os.path.join(str(tmp_path), f"rank{r}.json"))) for r in range(world)]


class Whole:
    """one context holding the whole SRS: what every rank must reproduce"""

    def __init__(self, log_n):
        import typlonk_amd
        from dist_compact_worker import SECRET, Witness
        from test_gpu_compact import _g2s
        from typlonk_amd.circuits import SquaringChain, fr_mont_limbs

        self.log_n, self.n = log_n, 1 << log_n
        self.ctx = typlonk_amd.Context(0)
        self.sid = self.ctx.srs_generate(fr_mont_limbs(SECRET), self.n + 3)
        self.chain = SquaringChain(self.ctx, log_n)
        self.vk = self.ctx.circuit_vk(self.sid, self.chain.circuit, self.chain.cosets, _g2s())
        self.plain_w = Witness(self.ctx, log_n)
        self._plain = None

    def prove(self, w):
        """("ok", proof) or (ERR_UNSATISFIED, message, proof) in the worker's form"""
        from dist_compact_worker import attempt

        return attempt(lambda: self.ctx.prove_compact(self.sid, self.chain.circuit, w.bufs, w.pib, w.pi_len, self.chain.cosets))

    def plain(self):
        if self._plain is None:
            self._plain = self.prove(self.plain_w)
            assert self._plain[0] == "ok"
        return self._plain

    def close(self):
        self.ctx.close()


def _struct_dict(hexed):
    from typlonk_amd.capi import ProofCompact, compact_dict

    return compact_dict(ProofCompact.from_buffer_copy(bytes.fromhex(hexed["struct"])))


def _check_equal(ref, ranks, pi_lens):
    """the `equal` step of every rank against the whole-SRS context `ref`"""
    from dist_compact_worker import Witness, pi_values
    from dist_compact_worker import pi_lens as parse
    from typlonk_amd.capi import vk_from_bytes, vk_to_bytes

    n, log_n = ref.n, ref.log_n
    want_vk = vk_to_bytes(ref.vk).hex()
    want_cm = [[[int(v) for v in xy], int(f)] for xy, f in ref.ctx.circuit_commitments(ref.sid, ref.chain.circuit)]
    for k, pl in enumerate(parse(pi_lens, n)):
        pi = pi_values(n, pl, 100 * log_n + k)
        w = Witness(ref.ctx, log_n, pi, variant=k + 1)
        want = ref.prove(w)
        pic = w.pib.download() if w.pib is not None else None
        w.free()
        assert want[0] == "ok"
        for r, o in enumerate(ranks):
            got = o["equal"][k]
            assert got["pi_len"] == pl
            # the 9 points, 7 evaluations and 5 challenges (the struct's bytes) and the 656 wire bytes, both forms
            assert got["dev"] == want, (r, pl, got["dev"][:2])
            assert got["host"] == want, (r, pl, got["host"][:2])
        # ... and it verifies: the struct under the whole-SRS key, its 656 bytes under the key a rank produced
        rank_vk = vk_from_bytes(bytes.fromhex(ranks[-1]["vk"]))
        assert ref.ctx.verify_compact(ref.vk, [_struct_dict(ranks[0]["equal"][k]["dev"][1])], [pic]).tolist() == [True]
        assert ref.ctx.verify_compact_bytes(rank_vk, bytes.fromhex(ranks[-1]["equal"][k]["dev"][1]["wire"]), [pic]).tolist() == [True]
    for r, o in enumerate(ranks):
        assert o["equal_cached"] == ref.plain(), r                       # once more, on the cached partial sums
        assert o["after_vk"] == ref.plain(), r
        assert o["vk"] == want_vk and o["vk_uncached"] == want_vk, r     # every rank's key is the whole-SRS key
        assert o["commitments"] == want_cm, r


def _check_failures(ref, ranks, world):
    from typlonk_amd.capi import ERR_COMM, ERR_HIP, ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE, ERR_UNSATISFIED, vk_to_bytes

    from dist_compact_worker import Witness

    bad = Witness(ref.ctx, ref.log_n, break_row=(ref.n - 3) // 2)
    want_unsat = ref.prove(bad)
    bad.free()
    assert want_unsat[0] == ERR_UNSATISFIED and want_unsat[2] is not None
    ok = ref.plain()
    want_vk = vk_to_bytes(ref.vk).hex()

    def one_fails(o, r, key, failing, code):
        got = o[key]
        if r == failing:
            assert got[0] == code, (r, key, got[:2])
        else:
            assert got[0] == ERR_COMM and f"rank {failing}" in got[1], (r, key, got[:2])

    for r, o in enumerate(ranks):
        # the last rank's first fold (12 records) loses its staging copy
        if r == world - 1:
            assert o["staging"][0] == ERR_HIP and "staging" in o["staging"][1], o["staging"][:2]
        else:
            assert o["staging"][0] == ERR_COMM and f"rank {world - 1}" in o["staging"][1] and "stage" in o["staging"][1], o["staging"][:2]
        assert o["staging_next"] == ok, r
        # an unsatisfied witness: all four folds complete, the same code and the same filled proof everywhere
        assert o["unsat"][0] == ERR_UNSATISFIED and o["unsat"][2] == want_unsat[2], (r, o["unsat"][:2])
        assert o["unsat_next"] == ok, r
        one_fails(o, r, "short_wire", 1, ERR_RANGE)
        assert o["short_wire_next"] == ok, r
        one_fails(o, r, "pi_long", 1, ERR_LENGTH)
        assert o["pi_long_next"] == ok, r
        one_fails(o, r, "vk_fail", 1, ERR_INVALID_ARG)
        assert o["vk_fail_next"] == want_vk, r
        # caches that differ between the ranks while a peer refuses its arguments
        one_fails(o, r, "cache_a1", 1, ERR_RANGE)
        assert o["cache_a2"] == ok, r
        if r == 1:
            assert o["cache_b1"][0] == ERR_COMM and "rank 0" in o["cache_b1"][1], o["cache_b1"][:2]
        else:
            assert o["cache_b1"][0] == ERR_RANGE, (r, o["cache_b1"][:2])
        one_fails(o, r, "cache_b2", 0, ERR_RANGE)
        assert o["cache_b3"] == ok, r


@pytest.mark.parametrize("world,log_n,tables", [(2, 10, False), (8, 10, False), (2, 12, False), (8, 12, False), (2, 15, True)])
def test_compact_proof_on_shards_equals_the_whole_srs_proof(built, tmp_path, world, log_n, tables):
    """typlonk_prove_compact and typlonk_prove_compact_host on every rank of `world` equal the proof of one context holding the
    whole SRS -- all 9 points, 7 evaluations and 5 challenges --, with pi_len 0, 1 and n, with the circuit commitments uncached
    and cached; every rank's typlonk_circuit_vk is the whole-SRS key through typlonk_vk_to_bytes (also when the key is the
    first call on a circuit), typlonk_circuit_commitments the whole-SRS commitments; the proof passes typlonk_verify_compact
    and its 656 bytes typlonk_verify_compact_bytes under the key a rank produced.  Without the feature every rank's first call
    returns TYPLONK_ERR_INVALID_ARG."""
    ranks = _ranks(world, log_n, tmp_path, ["equal"], tables=tables)
    ref = Whole(log_n)
    try:
        _check_equal(ref, ranks, "0,1,n")
    finally:
        ref.close()


@pytest.mark.parametrize("world,log_n", [(2, 10), (8, 12)])
def test_failures_leave_every_rank_at_the_same_collective(built, tmp_path, world, log_n):
    """Injected argument and copy errors the library is designed to survive, each followed by a proof that succeeds and equals
    the whole-SRS proof:
      * the last rank loses the staging copy of its first fold (TYPLONK_TEST_COMM_FAIL_STAGING in the test build of the
        library): it gets TYPLONK_ERR_HIP, the others TYPLONK_ERR_COMM naming it;
      * an unsatisfied witness: TYPLONK_ERR_UNSATISFIED on every rank with `out` equal to the single-context one;
      * rank 1 passes a wire buffer shorter than n (TYPLONK_ERR_RANGE there, TYPLONK_ERR_COMM naming rank 1 elsewhere), then
        pi_len > n (TYPLONK_ERR_LENGTH), then an unknown circuit inside typlonk_circuit_vk (TYPLONK_ERR_INVALID_ARG);
      * ranks whose circuit commitments are cached while a peer refuses its arguments, and the reverse: the record counts
        of the first fold do not depend on either."""
    ranks = _ranks(world, log_n, tmp_path, ["staging", "unsat", "fail", "cache"])
    ref = Whole(log_n)
    try:
        _check_failures(ref, ranks, world)
    finally:
        ref.close()


def test_shards_loaded_from_a_compressed_srs(built, tmp_path):
    """every rank takes its slice of a compressed SRS (typlonk_srs_load_compressed + typlonk_srs_set_shard; rank 0's slice
    holds P0): the same proof and the same key"""
    log_n = 10
    ref = Whole(log_n)
    try:
        def write_srs():
            with open(os.path.join(str(tmp_path), "srs.bin"), "wb") as f:
                f.write(ref.ctx.srs_download_compressed(ref.sid))

        ranks = _ranks(3, log_n, tmp_path, ["equal"], srs="bytes", prepare=write_srs)
        _check_equal(ref, ranks, "0,1,n")
    finally:
        ref.close()


def test_refusals_that_stay(built):
    """in one process: a shard WITHOUT a communicator is refused by the five calls that fold (nothing can fold mid-call from
    outside); typlonk_verify, typlonk_prove_batch and typlonk_prove_batch_compact refuse a shard with or without one.  With a
    one-rank communicator over the real RCCL, ShardedMsm.load_srs_compressed + ShardedProver.prove_compact / _host / circuit_vk
    return the whole-SRS results."""
    import torch

    from dist_compact_worker import Witness
    from test_gpu_compact import _g2s
    from typlonk_amd.capi import ERR_INVALID_ARG, TyplonkError, comm_available, comm_unique_id, vk_to_bytes
    from typlonk_amd.dist import ShardedMsm, ShardedProver

    log_n = 10
    n = 1 << log_n
    ref = Whole(log_n)
    ctx, chain, cosets, w = ref.ctx, ref.chain, ref.chain.cosets, ref.plain_w
    try:
        sh = ShardedMsm(ctx, n + 3, 0, 1, torch.device("cuda", 0))
        shard = sh.load_srs_compressed(ctx.srs_download_compressed(ref.sid))
        cols, _ = w.host()
        good = ctx.prove_compact(ref.sid, chain.circuit, w.bufs, None, 0, cosets)
        six = ctx.prove_native(ref.sid, chain.circuit, w.bufs, None, cosets)       # a reference-shape proof for typlonk_verify

        def refused(fn, *needles):
            with pytest.raises(TyplonkError) as e:
                fn()
            assert e.value.code == ERR_INVALID_ARG, str(e.value)
            for s in needles:
                assert s in str(e.value), str(e.value)

        def all_refuse_batches_and_verify():
            refused(lambda: ctx.verify(shard, chain.circuit, _g2s(), cosets, [six]), "one GPU")
            refused(lambda: ctx.prove_batch(shard, chain.circuit, [w.bufs], None, cosets), "one GPU")
            refused(lambda: ctx.prove_batch_compact(shard, chain.circuit, [w.bufs], None, None, cosets), "one GPU")

        # ---- no communicator ----
        refused(lambda: ctx.prove_compact(shard, chain.circuit, w.bufs, None, 0, cosets), "communicator")
        refused(lambda: ctx.prove_compact_host(shard, chain.circuit, cols, None, cosets), "communicator")
        refused(lambda: ctx.circuit_vk(shard, chain.circuit, cosets, _g2s()), "communicator")
        refused(lambda: ctx.circuit_commitments(shard, chain.circuit), "communicator")
        all_refuse_batches_and_verify()
        assert ctx.prove_compact(ref.sid, chain.circuit, w.bufs, None, 0, cosets)["witness"][0][0].tolist() == good["witness"][0][0].tolist()
        # ---- a one-rank communicator (the real librccl) ----
        if not comm_available():
            pytest.fail("librccl cannot be loaded: the one-rank collective path cannot run")
        ctx.comm_init(comm_unique_id(), 0, 1)
        all_refuse_batches_and_verify()
        from dist_compact_worker import proof_hex

        prover = ShardedProver(sh)
        assert proof_hex(prover.prove_compact(chain.circuit, w.bufs, None, 0, cosets)) == proof_hex(good)
        assert proof_hex(prover.prove_compact_host(chain.circuit, cols, None, cosets)) == proof_hex(good)
        assert vk_to_bytes(prover.circuit_vk(chain.circuit, cosets, _g2s())) == vk_to_bytes(ref.vk)
        ctx.comm_destroy()
    finally:
        ref.close()


@pytest.mark.slow
def test_eight_ranks_compact_at_2_20(built, tmp_path):
    """the full-size case: eight ranks share the GPU at 2^20 rows, 2^17-point shards with the library's own table choice; the
    compact proof (pi_len 0 and 1, device and host form, uncached and cached) and the key equal the whole-SRS ones"""
    from conftest import need_resources

    # per rank: a 2^17-point shard with c = 17 tables (~0.2 GiB), the 19 n Fr arena and the 4n coset tables of the circuit
    # (~1.9 GiB), the NTT tables; the parent holds the whole SRS beside them
    need_resources(host_gib=16, hbm_gib=40)
    ranks = _ranks(8, 20, tmp_path, ["equal"], tables=True, pi_lens="0,1", timeout=1500)
    ref = Whole(20)
    try:
        _check_equal(ref, ranks, "0,1")
    finally:
        ref.close()


@pytest.mark.parametrize("world", [2, 8])
def test_mirror_prove_compact_on_shards_from_plain_cpp_processes(built, tmp_path, world):
    """no Python in the ranks: tests/cpp/test_compact_ranks_host forks `world` copies of itself before touching the GPU; each
    is a rank on GPU 0 whose mirror (plonk::CompiledCircuit::prove_compact and the key on a sharded backend) must equal the
    whole-SRS proof and key it also computes, and verify_compact must accept the proof under the rank's key"""
    fake = os.path.join(ROOT, "tests", "cpp", "libfake_rccl.so")
    exe = os.path.join(ROOT, "tests", "cpp", "test_compact_ranks_host")
    env = dict(os.environ, TYPLONK_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_S="300")
    r = subprocess.run([exe, str(world), str(tmp_path)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and f"all {world} ranks ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
