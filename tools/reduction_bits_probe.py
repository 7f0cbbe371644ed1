"""Outputs of every kernel that reduces across lanes or waves (xerus_amd/csrc/reduce_dev.hpp), one .npy per output
under OUTDIR: arrays as they come, scalars as 1-element float64 arrays, ranks / statuses / iteration counts as ints.
The inputs are seeded and sensitive to re-association (standard normal entries times 2^k, k uniform in -20 .. 20;
lengths over more than one wave with a ragged tail), so a build that combines partial sums in another order
gives other bits. Run it on two library builds (XRS_LIB_PATH) and compare the directories byte by byte:
    python tools/reduction_bits_probe.py OUTDIR
The fused fp32 zipper reads XRS_ZIP32 once per process: dot_f32 under XRS_ZIP32=1 and 2 runs in a child process each.
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import xerus_ref as ref   # noqa: E402
from xerus_amd import capi, dist as xd   # noqa: E402

OUT = None


def save(name, value):
    a = np.asarray(value)
    if a.dtype.kind in "iub":
        a = a.astype(np.int64)
    elif a.dtype != np.float32:
        a = a.astype(np.float64)
    a = np.atleast_1d(a)
    np.save(os.path.join(OUT, name + ".npy"), a)
    shown = a.ravel()[0] if a.size == 1 else "%s %s" % (a.dtype, a.shape)
    print("%-40s %s" % (name, repr(shown) if a.size == 1 else shown), flush=True)


def wild(rng, shape):
    """standard normal entries times 2^k, k uniform in -20 .. 20"""
    return np.ldexp(rng.standard_normal(shape), rng.integers(-20, 21, size=shape))


def loaded_library():
    """the mapped builds of the C library, relative to the repository (one: the host API binds to the loaded one)"""
    names = {os.path.basename(capi.LIB_PATH), "libxerus_amd.so"}
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if os.path.basename(line.split()[-1]) in names}
    return sorted(os.path.relpath(p, ROOT) for p in paths)


def tt_pair(h, rng):
    d, n, r = 6, 4, 20
    ranks = [1] + [r] * (d - 1) + [1]
    make = lambda: [wild(rng, (ranks[k], n, ranks[k + 1])) for k in range(d)]   # noqa: E731
    return capi.TTDevice.from_cores(h, make()), capi.TTDevice.from_cores(h, make())


def zip32_child(tag):
    h = capi.Handle(0)
    x, y = tt_pair(h, np.random.default_rng(71))
    save("ttdot_f32_zip32_" + tag, x.dot_f32(y))
    h.close()


def elementwise(h, rng):
    for n in (1000, 70001):
        x, y = h.array(wild(rng, n)), h.array(wild(rng, n))
        save(f"nrm2_{n}", h.nrm2(x))
        save(f"dot_{n}", h.dot(x, y))
        save(f"asum_{n}", h.asum(x))


def factorisations(h, rng):
    for m, n in ((200, 12), (12, 200)):
        A = wild(rng, (m, n))
        for name in ("qr", "rq"):
            X, Y = getattr(h, name)(h.array(A))
            save(f"{name}_{m}x{n}_0", X.numpy())
            save(f"{name}_{m}x{n}_1", Y.numpy())
        for name in ("qc", "cq"):
            X, Y, rank = getattr(h, name)(h.array(A))
            save(f"{name}_{m}x{n}_0", X.numpy())
            save(f"{name}_{m}x{n}_1", Y.numpy())
            save(f"{name}_{m}x{n}_rank", rank)
    A = wild(rng, (96, 7)) @ rng.standard_normal((7, 96))
    Q, Cm, rank = h.qc(h.array(A))
    save("qc_rank7_0", Q.numpy())
    save("qc_rank7_1", Cm.numpy())
    save("qc_rank7_rank", rank)


def svds(h, rng):
    for m, n in ((96, 96), (129, 129), (300, 40)):
        U, S, Vt = h.svd(h.array(wild(rng, (m, n))))
        for part, a in (("U", U), ("S", S), ("Vt", Vt)):
            save(f"svd_{m}x{n}_{part}", a.numpy())
    U, S, Vt, st = h.svd_batched(h.array(wild(rng, (8, 24, 16))))
    for part, a in (("U", U), ("S", S), ("Vt", Vt)):
        save(f"svd_batched_{part}", a.numpy())
    save("svd_batched_status", st)
    A = h.array(wild(rng, (64, 64)))
    for kernel in (0, 1):
        S, Vt, sweeps = h.svd_rows_vt(A, kernel)
        save(f"svd_rows_vt_k{kernel}_S", S.numpy())
        save(f"svd_rows_vt_k{kernel}_Vt", Vt.numpy())
        save(f"svd_rows_vt_k{kernel}_sweeps", sweeps)


def eigensolvers(h, rng):
    for n, kk in ((128, 32), (256, 64)):
        G = wild(rng, (n, n))
        lam, Ut, st = h.sym_eig_top(h.array(G + G.T), kk)
        save(f"sym_eig_top_{n}_lam", lam.numpy())
        save(f"sym_eig_top_{n}_Ut", Ut.numpy())
        save(f"sym_eig_top_{n}_status", st)
    G = wild(rng, (128, 128))
    d, e = h.sym_tridiag(h.array(G + G.T))
    save("sym_tridiag_128_d", d)
    save("sym_tridiag_128_e", e)


def solves(h, rng):
    G = wild(rng, (200, 200))
    A = G @ G.T
    A = 0.5 * (A + A.T) + np.trace(A) / 200 * np.eye(200)   # symmetric positive definite
    save("solve_spd_200", h.solve(h.array(A), h.array(wild(rng, (200, 3)))).numpy())
    save("solve_lsq_300x40", h.solve(h.array(wild(rng, (300, 40))), h.array(wild(rng, (300, 3))), least_squares=True).numpy())


def rounds(h):
    import test_round_ownership_gpu as T
    for name, (make, eps, _) in T.CASES.items():
        cores, target = make(ref)
        g = capi.TTDevice.from_cores(h, [c.copy() for c in cores])
        g.round(target, eps)
        print("round", name, h.last_round_path(), g.ranks, flush=True)
        save(f"round_{name}_ranks", g.ranks)
        for k, c in enumerate(g.cores()):
            save(f"round_{name}_{k}", c)
        g.free()
    d, world = 5, 3
    s = ref.tt_add(ref.TT.random_raw([1] * d, [2] * (d - 1), ref.Rng(51)), ref.TT.random_raw([1] * d, [2] * (d - 1), ref.Rng(52)))
    comm = xd.EmulatedComm(h, world)
    st = xd.ShardedTT(h, capi.TTDevice.from_cores(h, s.cores), [world] * d, world, 0)
    print("round sharded-decline", repr(st.round_sharded(3, comm)), st.ranks, flush=True)
    for k, c in enumerate(st.local.cores()):
        save(f"round_sharded-decline_{k}", c)
    st.local.free()
    comm.close()


def tt_products(h, rng):
    x, y = tt_pair(h, np.random.default_rng(71))
    save("ttdot", x.dot(y))
    save("ttdot_f32", x.dot_f32(y))
    save("frob_norm", x.frob_norm())
    x.move_core(0)
    save("frob_norm_canonical", x.frob_norm())
    A, B = wild(rng, (96, 72)).astype(np.float32), wild(rng, (72, 80)).astype(np.float32)
    Cm = h.array_f32(np.zeros((96, 80), dtype=np.float32))
    h.gemm_f32(Cm, 96, 80, 1.0, h.array_f32(A), 72, False, 72, h.array_f32(B), 80, False)
    save("gemm_f32_96x80x72", Cm.numpy())


def largest_entry(h, rng):
    d, n, r = 4, 6, 5
    ranks = [1] + [r] * (d - 1) + [1]
    x = capi.TTDevice.from_cores(h, [wild(rng, (ranks[k], n, ranks[k + 1])) for k in range(d)])
    sq = x.entrywise_square(0.75)
    save("entrywise_square_ranks", sq.ranks)
    for k, c in enumerate(sq.cores()):
        save(f"entrywise_square_{k}", c)
    # rank-one cores; the two longer ones span several waves (one workgroup per core), with tied maxima
    cores = [wild(rng, (1, m, 1)) for m in (n, n, 300, 70)]
    cores[2][0, [17, 150, 290], 0] = -np.abs(cores[2]).max() * 2.0
    save("rank_one_argmax", capi.TTDevice.from_cores(h, cores).rank_one_argmax())


def tangent(h, xe, rng):
    # xrs_tt_tangent_to_tt only assembles blocks; the certificate and the sums of tangent.hip are reached by the
    # projection (k_tangent_cert) and the scalar product (k_tangent_dot) of the host API, at the first case of
    # tests/test_tangent_gpu.py
    import test_tangent_gpu as T
    n, r = [3, 4, 2], [1, 1, 1, 1]
    U = [wild(rng, (r[k], n[k], r[k + 1])) for k in range(3)]
    V = [wild(rng, (r[k], n[k], r[k + 1])) for k in range(3)]
    for k, c in enumerate(h.tangent_to_tt(n, r, [h.array(c) for c in U], [h.array(c) for c in V], True)):
        save(f"tangent_to_tt_{k}", c.numpy())
    dims, ranks, zranks, seed = T.CASES[0]
    trng = np.random.default_rng(seed)
    X = T._tt(xe, T._random_cores(trng, dims, ranks))
    X.move_core(0)
    tv = xe.TTTangentVector(X, T._tt(xe, T._random_cores(trng, dims, zranks)))
    tv2 = xe.TTTangentVector(X, T._tt(xe, T._random_cores(trng, dims, zranks)))
    for k, c in enumerate(tv.components):
        save(f"tangent_component_{k}", c.to_ndarray())
    save("tangent_fallback_edges", tv.fallbackEdges)
    save("tangent_scalar_product", tv.scalar_product(tv2))
    save("tangent_frob_norm", tv.frob_norm())


def uq(h):
    # the smallest shape of tests/test_uq_kernels_gpu.py is one sample of rank 1: the sums are reached with more
    # than one sample per thread only from N = 257, the test's other sample count, at its second shape (3, 5)
    import test_uq_kernels_gpu as T
    for N, a, n, b in ((1, 1, 1, 1), (257, 3, 4, 5)):
        X, P, L, V = T._inputs(N, a, n, b, seed=a * 1000 + b * 10 + n)
        for with_l in (False, True):
            dL = h.array(L) if with_l else None
            save(f"uq_quadform_N{N}_a{a}_L{int(with_l)}", h.uq_quadform(dL, h.array(V)))
            save(f"uq_stack_congruence_N{N}_a{a}_b{b}_L{int(with_l)}", h.uq_stack_congruence(dL, h.array(X), h.array(P)).numpy())


def adf(xe):
    """one sweep of test_adf_matches_oracle_fixed_rank, single-point and rank-one measurements"""
    import test_adf_gpu as T
    for kind in ("sp", "r1"):
        rng = ref.Rng(31)
        D, N, R = 5, 4, 2
        true = ref.TT.random([N] * D, [R] * (D - 1), rng)
        pos = ref.sp_random_positions(rng, 300, [N] * D)
        vals = ref.tt_measure_sp(true, pos)
        x = T._tt_from(xe, ref.TT.random_raw([N] * D, [R] * (D - 1), rng).cores)
        meas = T._sp_set(xe, pos, vals)
        res = xe.ADFVariant(1, 1e-14, 1.0)(x, meas if kind == "sp" else xe.RankOneMeasurementSet(meas, [N] * D))
        save(f"adf_{kind}_residual", res)
        for k in range(D):
            save(f"adf_{kind}_{k}", x.get_component(k).to_ndarray())


def als_local(h, rng):
    import als_local_ref as lr
    dims = (5, 4, 6, 3, 3)
    p = lr.problem(dims, False)
    L, A, R = h.array(p.L), h.array(p.A), h.array(p.R)
    b = h.array(wild(rng, dims[:3]))
    for check_every in (1, 16):
        x = h.array(p.x0)
        iters, relres, status = h.als_local_cg(x, b, dims, L, A, R, False, 1e-10, 0, check_every)
        save(f"als_local_cg_ce{check_every}_x", x.numpy())
        save(f"als_local_cg_ce{check_every}_iters", iters)
        save(f"als_local_cg_ce{check_every}_relres", relres)
        save(f"als_local_cg_ce{check_every}_status", status)
        x = h.array(p.x0)
        theta, iters, relres, status = h.als_local_eig(x, dims, L, A, R, 1e-10, 0, check_every)
        save(f"als_local_eig_ce{check_every}_x", x.numpy())
        save(f"als_local_eig_ce{check_every}_theta", theta)
        save(f"als_local_eig_ce{check_every}_iters", iters)
        save(f"als_local_eig_ce{check_every}_relres", relres)
        save(f"als_local_eig_ce{check_every}_status", status)


def main():
    global OUT
    OUT = sys.argv[1]
    os.makedirs(OUT, exist_ok=True)
    if len(sys.argv) > 2:
        return zip32_child(sys.argv[2])
    h = capi.Handle(0)
    import xerus_amd.xerus as xe   # (after the C library: the module binds to the libxerus_amd that is loaded)
    xe.seed(0xBAADF00D)
    print("library:", *loaded_library(), flush=True)
    rng = np.random.default_rng(2015)
    elementwise(h, rng)
    factorisations(h, rng)
    svds(h, rng)
    eigensolvers(h, rng)
    solves(h, rng)
    rounds(h)
    tt_products(h, rng)
    largest_entry(h, rng)
    tangent(h, xe, rng)
    uq(h)
    adf(xe)
    als_local(h, rng)
    h.close()
    for tag in ("1", "2"):
        subprocess.run([sys.executable, os.path.abspath(__file__), OUT, tag], env=dict(os.environ, XRS_ZIP32=tag), check=True)


if __name__ == "__main__":
    main()
