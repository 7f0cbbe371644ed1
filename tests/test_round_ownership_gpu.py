"""Who owns a round's candidate cores: every exit of the three device-resident rounds (chain, certified
truncation, general), by a return or by a throw, gives the blocks it allocated back to the handle's pool.

Steady pool: the same round repeated on one handle holds the same number of pool bytes after iterations 2, 3
and 4 (iteration 1 warms the cache), on every path: adopted (chain / truncate / general, the last also after the
first two declined), declined by all three (reference), declined when sharded (path "").

A throw in mid-round: a one-rank all-reduce hook that fails on its n-th call makes the sharded round raise
("all-reduce callback failed", a host status) at every all-reduce of the chain and of the truncating round
in turn; the TT is untouched, the pool does not grow from one failure to the next, and a clean round on the
same handle afterwards gives what a fresh handle gives. (Before the rounds had one owner for their candidate
cores the pool grew after a failure at call 5 of 5 of the chain round and at calls 6..11 of 11 of the truncating
round: every all-reduce behind the allocation of the new cores, profiles/r12/ownership.txt.)
"""
import ctypes as C

import numpy as np
import pytest

from xerus_amd import capi
from xerus_amd import dist as xd

pytestmark = pytest.mark.gpu

EPSILON = 8 * np.finfo(float).eps


@pytest.fixture
def own_handle(handle):
    """A handle of this test's own (an empty pool); `handle` only for its skip without a GPU."""
    h = capi.Handle(0)
    yield h
    h.close()


def _chain(ref):
    return ref.TT.random([4, 5, 3, 4, 2], [3, 6, 5, 2], ref.Rng(11)).cores, 6


def _truncate(ref):
    return ref.TT.random([6] * 5, [20] * 4, ref.Rng(13)).cores, 7


def _general(ref):
    """test_graded_small: raw cores whose right rank index is scaled by 0.7^j (no Gram certificate holds)."""
    x = ref.TT.random_raw([6] * 6, [20] * 5, ref.Rng(105 + 6))
    for k in range(5):
        x.cores[k] = x.cores[k] * (0.7 ** np.arange(x.cores[k].shape[2]))[None, None, :]
    return x.cores, 9


def _deficient(ref, edge):
    """test_round_certificate_fails_mid_sweep: the right unfolding of core `edge` cut to rank 2."""
    x = ref.TT.random_raw([5] * 5, [4, 6, 6, 4], ref.Rng(19))
    c = x.cores[edge]
    U, S, Vt = np.linalg.svd(c.reshape(c.shape[0], -1), full_matrices=False)
    S[2:] = 0.0
    x.cores[edge] = ((U * S) @ Vt).reshape(c.shape)
    return x.cores, 6


def _doubled(ref):
    """test_round_sum_recovers_ranks: x + x, every unfolding exactly rank-deficient (a QC rank drop at every edge)."""
    x = ref.TT.random([5, 4, 6, 3, 5], [4, 7, 6, 3], ref.Rng(17))
    return ref.tt_add(x, x).cores, 100


# (the rank-deficient interior core is cut by the general round after the chain and the certified truncation
# decline; the doubled TT is declined by all three and goes to the reference's sequential sweeps)
CASES = {
    "chain": (_chain, EPSILON, "chain"),
    "truncate": (_truncate, EPSILON, "truncate"),
    "general": (_general, 1e-10, "general"),
    "deficient-edge1": (lambda ref: _deficient(ref, 1), EPSILON, "general"),
    "deficient-edge3": (lambda ref: _deficient(ref, 3), EPSILON, "general"),
    "doubled": (_doubled, EPSILON, "reference"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_pool_steady(own_handle, ref, case):
    make, eps, expected = CASES[case]
    cores, target = make(ref)
    held = []
    for _ in range(4):
        g = capi.TTDevice.from_cores(own_handle, [c.copy() for c in cores])
        g.round(target, eps)
        assert own_handle.last_round_path() == expected
        g.free()
        held.append(own_handle.pool_bytes())
    print(case, held)
    assert held[1] == held[2] == held[3], held


def test_pool_steady_sharded_decline(own_handle, ref):
    """test_emulated_comm_tall_right_edge_reports_uncertified's input: every sharded round declines (path "")."""
    d, world = 5, 3
    s = ref.tt_add(ref.TT.random_raw([1] * d, [2] * (d - 1), ref.Rng(51)), ref.TT.random_raw([1] * d, [2] * (d - 1), ref.Rng(52)))
    comm = xd.EmulatedComm(own_handle, world)
    try:
        held = []
        for _ in range(4):
            st = xd.ShardedTT(own_handle, capi.TTDevice.from_cores(own_handle, [c.copy() for c in s.cores]), [world] * d, world, 0)
            assert st.round_sharded(3, comm) == ""
            st.local.free()
            held.append(own_handle.pool_bytes())
        print("sharded decline", held)
        assert held[1] == held[2] == held[3], held
    finally:
        comm.close()


class FailingAllReduce:
    """One rank's all-reduce hook (the local sum is the global sum): status 0, and 1 on call number `fail_at`."""

    def __init__(self, fail_at: int = 0):
        self.calls, self.fail_at, self.ctx = 0, fail_at, None

        def _cb(_ctx, _ptr, _count):
            self.calls += 1
            return 1 if self.calls == self.fail_at else 0

        self.fn = xd.ALLREDUCE_FN(_cb)   # (a reference: the C side only holds the pointer)

    @property
    def c_fn(self):
        return C.cast(self.fn, C.c_void_p)


def _sharded(h, cores):
    dims = [c.shape[1] for c in cores]
    return xd.ShardedTT(h, capi.TTDevice.from_cores(h, [c.copy() for c in cores]), dims, 1, 0)


def _clean_round(h, ref, cores, target):
    st = _sharded(h, cores)
    hook = FailingAllReduce()
    path = st.round_sharded(target, hook)
    out = (path, list(st.ranks), ref.TT(st.local.cores()).full(), hook.calls)
    st.local.free()
    return out


# inputs without structural excess at the left end (r_{k+1} <= r_k n_k: the round's first step changes no core)
THROW_CASES = {
    "chain": ([4, 5, 3, 4, 2], [3, 6, 5, 2], 6),
    "truncate": ([6] * 5, [6, 12, 12, 6], 4),
}


@pytest.mark.parametrize("case", list(THROW_CASES))
def test_throw_in_mid_round_releases_everything(handle, ref, case):
    dims, ranks, target = THROW_CASES[case]
    x = ref.TT.random(dims, ranks, ref.Rng(71))
    before = ref.TT([c.copy() for c in x.cores]).full()
    fresh = capi.Handle(0)
    try:
        path, ranks0, full0, ncalls = _clean_round(fresh, ref, x.cores, target)
    finally:
        fresh.close()
    assert path == case and ncalls >= len(dims) - 1, (path, ncalls)
    growing = []
    for n in range(1, ncalls + 1):
        h = capi.Handle(0)
        try:
            held = []
            for _ in range(3):
                st = _sharded(h, x.cores)
                ranks_in = list(st.ranks)
                with pytest.raises(capi.XrsError, match="all-reduce callback failed"):
                    st.round_sharded(target, FailingAllReduce(n))
                assert list(st.ranks) == ranks_in, (n, st.ranks)
                after = ref.TT(st.local.cores()).full()
                assert np.linalg.norm(after - before) <= 1e-12 * np.linalg.norm(before), n
                st.local.free()
                held.append(h.pool_bytes())
            if held[1] != held[2]:
                growing.append((n, held))
            path1, ranks1, full1, _ = _clean_round(h, ref, x.cores, target)
            assert (path1, ranks1) == (path, ranks0), n
            assert np.linalg.norm(full1 - full0) <= 1e-10 * np.linalg.norm(full0), n
        finally:
            h.close()
    print(case, "all-reduce calls of a clean round:", ncalls, "pool grows after a failure at call:", growing)
    assert not growing, growing
