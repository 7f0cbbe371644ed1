"""The two lanes of the certified round's chain pass: between the batched Cholesky and the
deviations the main lane keeps only the largest same-shape group of each stage; the explicit inverses and the
boundary cores' transforms and Grams run on side stream 0.

Nothing in the arithmetic changes, so the checks are byte comparisons: against the same round with the lanes
serialised (inside prof_begin / prof_end every launch goes to the main stream in program order), between
repeats (a lane race shows as nondeterminism), and with the pool's released blocks overwritten at once (a
temporary given back before the other lane's last reader was joined shows as a changed core). The degenerate
groupings (all shapes different, d = 2 and 3), a rank-deficient input, an input that needs the second pass and
the asynchronous inner product beside the round are checked against the oracle with the tolerances of
tests/test_tt_gpu.py for the same quantities.

Shapes: boundary groups beside an interior group, both GEMM kernels reached --
order 8, n = 4, maximal ranks up to 64 (1, 4, 16, 64, 64, 64, 16, 4, 1), and order 6, n = 20, rank 32
(boundary K = 20, no multiple of 32). By its size rule the round keeps passes this small on one lane (the event
hops would cost more than the lanes hide), so every test here switches all three stages on with
XRS_ROUND_LANES=7, which the library reads at each pass; test_bench_shape_default runs the shape at which the
rule itself chooses the lanes.
"""
import numpy as np
import pytest

from xerus_amd import capi

pytestmark = pytest.mark.gpu

SHAPES = {
    "o8n4r64": ([4] * 8, [4, 16, 64, 64, 64, 16, 4]),
    "o6n20r32": ([20] * 6, [20, 32, 32, 32, 20]),
}
PROF_ALL = 0xFFFFFFFF

_inputs = {}


@pytest.fixture(autouse=True)
def all_lanes(monkeypatch):
    monkeypatch.setenv("XRS_ROUND_LANES", "7")


def _input(ref, name):
    """One canonical random TT per shape (TTTensor::random: raw cores, move_core(0)), shared and never modified."""
    if name not in _inputs:
        dims, ranks = SHAPES[name]
        x = ref.TT.random(dims, ranks, ref.Rng(7))
        assert x.ranks == ranks
        _inputs[name] = x
    return _inputs[name]


def _same_bytes(a_cores, b_cores):
    return len(a_cores) == len(b_cores) and all(a.shape == b.shape and a.tobytes() == b.tobytes()
                                                for a, b in zip(a_cores, b_cores))


def _check_against_oracle(ref, handle, x, target, chain=True):
    """Rounds x on the GPU and in the oracle: same ranks, same tensor as the input, right-orthonormal cores."""
    from ttutil import tt_diff_norm

    g = capi.TTDevice.from_cores(handle, [c.copy() for c in x.cores])
    g.round(target)
    path = handle.last_round_path()
    y = x.copy()
    y.round(target)
    assert g.ranks == y.ranks
    gc = g.cores()
    g.free()
    diff, nrm = tt_diff_norm(gc, x.cores)
    print("path", path, "ranks", g.ranks, "rel diff %.3e" % (diff / nrm))
    assert diff <= 1e-10 * nrm
    for c in gc[1:]:
        M = c.reshape(c.shape[0], -1)
        assert np.linalg.norm(M @ M.T - np.eye(M.shape[0])) <= 1e-12 * M.shape[0]
    if chain:
        assert path == "chain"
    return path, gc


@pytest.mark.parametrize("shape", list(SHAPES))
def test_serialised_reference(handle, ref, shape):
    """The cores of a certified round are byte for byte those of the same round with the lanes serialised."""
    x = _input(ref, shape)
    target = max(SHAPES[shape][1])
    g = capi.TTDevice.from_cores(handle, [c.copy() for c in x.cores])
    g.round(target)
    assert handle.last_round_path() == "chain"
    two_lanes = g.cores()
    g.free()
    s = capi.TTDevice.from_cores(handle, [c.copy() for c in x.cores])
    handle.prof_begin(PROF_ALL)
    try:
        s.round(target)
    finally:
        stats = handle.prof_end()
    assert handle.last_round_path() == "chain"
    assert stats["launches"] > 0
    one_lane = s.cores()
    s.free()
    assert s.ranks == g.ranks == SHAPES[shape][1]
    assert _same_bytes(two_lanes, one_lane)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_repeats(handle, ref, shape):
    """Ten rounds of clones of one input return byte-identical cores."""
    x = _input(ref, shape)
    target = max(SHAPES[shape][1])
    base = capi.TTDevice.from_cores(handle, [c.copy() for c in x.cores])
    first = None
    for i in range(10):
        g = base.clone()
        g.round(target)
        assert handle.last_round_path() == "chain"
        out = g.cores()
        g.free()
        if first is None:
            first = out
        else:
            assert _same_bytes(first, out), i
    base.free()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_pool_reuse(handle, ref, shape):
    """The same when, right after each round returns, blocks of every size the round gave back to the pool (the
    old cores, L_k, Z_k, W_k, the Gram slab, the statuses) are taken again and filled with NaN before the cores
    are read: a block that a lane still used when it was released would be overwritten under it."""
    dims, ranks = SHAPES[shape]
    x = _input(ref, shape)
    target = max(ranks)
    r = [1] + ranks + [1]
    core_sizes = [r[k] * dims[k] * r[k + 1] for k in range(len(dims))]
    squares = [a * a for a in ranks]
    sizes = core_sizes * 2 + squares * 3 + [sum(squares) + 16 * len(ranks), 64]
    nan_blocks = [np.full(n, np.nan) for n in sizes]
    base = capi.TTDevice.from_cores(handle, [c.copy() for c in x.cores])
    first = None
    for i in range(10):
        g = base.clone()
        g.round(target)
        junk = [handle.array(b) for b in nan_blocks]
        out = g.cores()
        for j in junk:
            j.free()
        g.free()
        assert all(np.isfinite(c).all() for c in out), i
        if first is None:
            first = out
        else:
            assert _same_bytes(first, out), i
    base.free()


def test_all_shapes_different(handle, ref):
    """Order 5, n = 2, 3, 4, 3, 2: every transform and every Gram is a group of its own, so the "largest group"
    of each stage is a single job."""
    x = ref.TT.random([2, 3, 4, 3, 2], [2, 5, 4, 2], ref.Rng(31))
    assert x.ranks == [2, 5, 4, 2]
    _check_against_oracle(ref, handle, x, 5)


@pytest.mark.parametrize("dims,ranks", [([5, 6], [4]), ([7, 3, 5], [6, 4])])
def test_short_trains(handle, ref, dims, ranks):
    """d = 2 (no inner core at all) and d = 3 (one inner core, no two jobs of one shape)."""
    x = ref.TT.random(dims, ranks, ref.Rng(37))
    _check_against_oracle(ref, handle, x, max(ranks))


def test_deficient_input(handle, ref):
    """A rank-deficient interior unfolding (tests/test_tt_gpu.py, test_round_certificate_fails_mid_sweep): a
    factorisation of the pass fails; its status is read behind the lanes' join, the chain result is discarded and
    the round reproduces the oracle's rank drop on another path."""
    x = ref.TT.random_raw([5, 5, 5, 5, 5], [4, 6, 6, 4], ref.Rng(19))
    c = x.cores[3]
    U, S, Vt = np.linalg.svd(c.reshape(c.shape[0], -1), full_matrices=False)
    S[2:] = 0.0
    x.cores[3] = ((U * S) @ Vt).reshape(c.shape)
    path, _ = _check_against_oracle(ref, handle, x, 6, chain=False)
    assert path is not None and path != "chain"


def test_second_pass(handle, ref):
    """Raw N(0,1) cores of order 6, n = 4 at ranks 4, 16, 16, 16, 4: the interface matrices X_{>=4} (16 x 16) and
    X_{>=5} (4 x 4) are square products of Gaussian matrices, kappa in the hundreds, still far inside the Gram
    certificate (lambda_min / trace ~ 1e-7 against the 1e-11 shift). A chain pass loses about kappa^2 u, so
    pass 1 misses the 1e-13 orthonormality bar and the round repeats the right chain on the pass-1 cores
    (certify = false) through the same lanes; boundary groups and the inner group k = 2, 3 coexist."""
    dims, ranks = [4] * 6, [4, 16, 16, 16, 4]
    x = ref.TT.random_raw(dims, ranks, ref.Rng(41))
    assert x.ranks == ranks
    kappa, R = 0.0, None
    for c in reversed(x.cores[1:]):   # X_{>=k}, k = d-1 .. 1
        R = c.reshape(c.shape[0], -1) if R is None else (c.reshape(-1, c.shape[2]) @ R).reshape(c.shape[0], -1)
        kappa = max(kappa, np.linalg.cond(R))
    print("largest condition number of a right interface matrix: %.1f" % kappa)
    assert 100 * 1e-13 < kappa * kappa * np.finfo(float).eps < 1e-8   # one pass misses the bar, two meet it
    _check_against_oracle(ref, handle, x, max(ranks))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_dot_async_beside_round(handle, ref, shape):
    """dot_async beside the round: the value is bit for bit the synchronous product's, and the round's cores
    are byte for byte those of a round without it."""
    dims, ranks = SHAPES[shape]
    x = _input(ref, shape)
    y = ref.TT.random(dims, ranks, ref.Rng(43))
    target = max(ranks)
    gy = capi.TTDevice.from_cores(handle, y.cores)
    alone = capi.TTDevice.from_cores(handle, [c.copy() for c in x.cores])
    d_sync = alone.dot(gy)
    nx, ny = np.sqrt(ref.dot(x, x)), np.sqrt(ref.dot(y, y))
    assert abs(d_sync - ref.dot(x, y)) <= 1e-12 * nx * ny
    alone.round(target)
    assert handle.last_round_path() == "chain"
    expect = alone.cores()
    alone.free()
    for i in range(3):
        g = capi.TTDevice.from_cores(handle, [c.copy() for c in x.cores])
        fut = g.dot_async(gy)
        g.round(target)
        d = fut.result()
        assert handle.last_round_path() == "chain"
        out = g.cores()
        g.free()
        assert d == d_sync, i
        assert _same_bytes(expect, out), i
    gy.free()


def test_bench_shape_default(handle, ref, monkeypatch):
    """Order 10, n = 20, rank 256 without the switch: the size rule turns the lanes on (4.0 GFLOP of batched right
    factors). Two-lane cores byte for byte the serialised ones, and the same from round to round."""
    monkeypatch.delenv("XRS_ROUND_LANES")
    x = ref.TT.random_raw([20] * 10, [256] * 9, ref.Rng(23))
    base = capi.TTDevice.from_cores(handle, x.cores)
    base.move_core(0)
    outs = []
    for i in range(4):
        g = base.clone()
        if i == 3:
            handle.prof_begin(PROF_ALL)
        try:
            g.round(256)
        finally:
            if i == 3:
                handle.prof_end()
        assert handle.last_round_path() == "chain"
        outs.append(g.cores())
        g.free()
    base.free()
    for i in (1, 2, 3):
        assert _same_bytes(outs[0], outs[i]), i
