"""Tangent-vector probe at the cfg3 shape (order 10, n = 20, base and direction rank 128): the projection onto
the tangent space (TTTangentVector(base, direction)), to_tt, scalar_product and one HOSVD retraction
(added_to_base().round(128)) through the tangent drivers, against the same projection written with indexed
Tensor expressions (the reference's own formulation, retractions.cpp:82-130, which needs nothing of the
tangent layer).

Every figure is the median of HIP-event times on the handle's stream (events recorded around the call, which
ends with its own synchronisation), after warm-up runs of the same shape.

    python tools/tangent_probe.py [--order 10 --n 20 --rank 128 --reps 15 --warmup 3] [--once projection]
--once NAME runs one warm-up and one evaluation of that step only (for a kernel trace).
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xerus_amd.xerus as xe  # noqa: E402

hip = ctypes.CDLL("libamdhip64.so")


def _hip(status):
    if status != 0:
        raise RuntimeError(f"HIP call failed with status {status}")


class Events:
    def __init__(self):
        self.start, self.stop = ctypes.c_void_p(), ctypes.c_void_p()
        _hip(hip.hipEventCreate(ctypes.byref(self.start)))
        _hip(hip.hipEventCreate(ctypes.byref(self.stop)))
        self.stream = ctypes.c_void_p(xe.stream())

    def time_ms(self, fn):
        xe.synchronize()
        _hip(hip.hipEventRecord(self.start, self.stream))
        out = fn()
        _hip(hip.hipEventRecord(self.stop, self.stream))
        _hip(hip.hipEventSynchronize(self.stop))
        ms = ctypes.c_float()
        _hip(hip.hipEventElapsedTime(ctypes.byref(ms), self.start, self.stop))
        return ms.value, out


def median_ms(ev, fn, warmup, reps):
    first = ev.time_ms(fn)[0]   # the first run is a warm-up; a step of seconds is then timed three times only
    if first > 200.0:
        warmup, reps = 0, 3
    for _ in range(max(0, warmup - 1)):
        fn()
    times = sorted(ev.time_ms(fn)[0] for _ in range(reps))
    return statistics.median(times), times[0], times[-1], reps


def random_tt(rng, dims, rank):
    d = len(dims)
    t = xe.TTTensor(dims)
    for k in range(d):
        shape = (1 if k == 0 else rank, dims[k], 1 if k == d - 1 else rank)
        t.set_component(k, xe.Tensor.from_ndarray(rng.standard_normal(shape) / np.sqrt(shape[0] * shape[1])))
    return t


def indexed_projection(X, Z):
    """retractions.cpp:82-130 with indexed Tensor expressions: the components of the projection of Z at X."""
    d = X.degree()
    i1, i2, j1, j2, r, s = xe.indices(6)
    one = xe.Tensor.from_ndarray(np.ones((1, 1)))
    UV, UU = [one], [one]
    for k in range(d - 1):
        U, Zk = X.get_component(k), Z.get_component(k)
        nv, nu = xe.Tensor(), xe.Tensor()
        nv(j1, j2) << UV[-1](i1, i2) * U(i1, r, j1) * Zk(i2, r, j2)
        nu(j1, j2) << UU[-1](i1, i2) * U(i1, r, j1) * U(i2, r, j2)
        UV.append(nv)
        UU.append(nu)
    right = one
    comps = [None] * d
    for k in range(d - 1, -1, -1):
        U, Zk = X.get_component(k), Z.get_component(k)
        inv = xe.pseudo_inverse(UU[k], 1)
        V = xe.Tensor()
        V(i1, r, j1) << inv(i1, s) * UV[k](s, i2) * Zk(i2, r, j2) * right(j1, j2)
        if k != 0:
            UTV, W, nr = xe.Tensor(), xe.Tensor(), xe.Tensor()
            UTV(i1, i2) << V(i1, r, j1) * U(i2, r, j1)
            W(i1, r, j1) << V(i1, r, j1) - UTV(i1, s) * U(s, r, j1)
            V = W
            nr(j1, j2) << U(j1, r, i1) * Zk(j2, r, i2) * right(i1, i2)
            right = nr
        comps[k] = V
    return comps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--order", type=int, default=10)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--rank", type=int, default=128)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", default=None, choices=["projection", "to_tt", "scalar_product", "hosvd", "added_to_base", "round_only", "indexed"])
    a = ap.parse_args()
    dims = [a.n] * a.order
    rng = np.random.default_rng(0)
    X = random_tt(rng, dims, a.rank)
    X.move_core(0)
    Z = random_tt(rng, dims, a.rank)
    Z2 = random_tt(rng, dims, a.rank)
    tv, tv2 = xe.TTTangentVector(X, Z), xe.TTTangentVector(X, Z2)
    block = tv.added_to_base()
    steps = {
        "projection": lambda: xe.TTTangentVector(X, Z),
        "to_tt": lambda: tv.to_tt(),
        "scalar_product": lambda: tv.scalar_product(tv2),
        "hosvd": lambda: tv.added_to_base().round(a.rank),
        "added_to_base": lambda: tv.added_to_base(),
        "round_only": lambda: xe.TTTensor(block).round(a.rank),
        "indexed": lambda: indexed_projection(X, Z),
    }
    if a.once:
        steps[a.once]()
        xe.synchronize()
        steps[a.once]()
        xe.synchronize()
        return
    print(f"tangent probe: order {a.order}, n {a.n}, rank {a.rank}; base ranks {X.ranks()}, fallback edges {tv.fallbackEdges}")
    # the two formulations agree (same gauge: both read the cores of X)
    worst = 0.0
    for got, want in zip(tv.components, indexed_projection(X, Z)):
        worst = max(worst, xe.frob_norm(got - want) / max(tv.frob_norm(), 1e-300))
    print(f"components, tangent driver against indexed composition: largest difference {worst:.2e} of the vector's norm")
    ev = Events()
    labels = {
        "projection": "projection TTTangentVector(base, direction)",
        "to_tt": "to_tt (block kernel + move_core(0) of the rank-2r TT)",
        "scalar_product": "scalar_product",
        "hosvd": f"HOSVD retraction added_to_base().round({a.rank})",
        "added_to_base": "  of which added_to_base() (block kernel + move_core(0))",
        "round_only": f"  of which round({a.rank}) of the rank-2r TT",
        "indexed": "projection, indexed Tensor composition (baseline)",
    }
    med = {}
    for name, fn in steps.items():
        med[name], lo, hi, runs = median_ms(ev, fn, a.warmup, a.reps)
        print(f"{labels[name]:62s} median {med[name]:9.3f} ms  (min {lo:.3f}, max {hi:.3f}, {runs} runs)")
        if name == "round_only":
            paths = {1: "chain", 2: "certified truncation", 3: "reference sweeps", 4: "general"}
            print(f"    ranks of the rank-2r TT {block.ranks()}; round path: {paths.get(xe.last_round_path(), 'none')}")
    print(f"projection speed-up over the indexed composition: {med['indexed'] / med['projection']:.2f}x")


if __name__ == "__main__":
    main()
