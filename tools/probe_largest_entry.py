"""find_largest_entry probe: the symmetric-square loop against the same loop on the Kronecker square.

For seeded normalised random TTs of order 16 with (mode size, rank) = (2, 8), (3, 16), (4, 24), accuracy 0.9 and
lowerBound = |T[p]| at the position p of the round(1) estimate:

  (a)  xe.find_largest_entry(T, 0.9, lowerBound): X o X by entrywise_square (ranks r (r + 1) / 2);
  (b)  the same loop (largestEntry.cpp:10-36, with the library's iteration guard) written here on the public API
       with xe.entrywise_product(X, X), the Kronecker form of rank r^2.

Wall clock around calls that end synchronised; (a) and (b) alternate in one process after a warm-up of each;
--reps repetitions, median and spread. Also printed: the largest rank before the rank-revealing QC that follows
the square (s(r) resp. r^2 of the largest rank entering a square; for (a) from an untimed replay of the loop with
xe.entrywise_square), the iterations, and whether the two positions agree. A variant that runs out of memory is
reported as such.

A replay stops before a square whose cores would take more than --max-gib (default 8 GiB) and says so: past that
the soft threshold that follows factors edges of rank in the thousands one by one, minutes per edge, whichever
square is used. When a replay stopped, there is no position to compare; the probe then times the first k
iterations both variants complete, (a) as this file's loop with xe.entrywise_square.

    python tools/probe_largest_entry.py [--sizes 2x8,3x16,4x24] [--reps 5] [--order 16] [--max-gib 8]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xerus_amd.xerus as xe  # noqa: E402

ACCURACY = 0.9


def rank_one_estimate(t):
    y = xe.TTTensor(t)
    y.round(1)
    return xe.find_largest_entry(y, 0.0, 0.0)


def square_bytes(x, pre_qc_rank):
    r = [1] + [pre_qc_rank(v) for v in x.ranks()] + [1]
    return 8 * sum(r[k] * n * r[k + 1] for k, n in enumerate(x.dimensions))


def loop(t, accuracy, lower_bound, square, pre_qc_rank, max_bytes, max_iterations=1000, log=None):
    """largestEntry.cpp:10-36 on the public API. Returns (position, iterations, largest rank before the QC, note):
    position is None when the loop was stopped (by max_bytes before a square, or after max_iterations)."""
    d = t.degree()
    alpha = accuracy
    xn = max(t[rank_one_estimate(t)], lower_bound)
    tau = (1 - alpha) * alpha * xn * xn / (2.0 * (d - 1))
    x = xe.TTTensor(t)
    iterations, widest = 0, 0
    while sum(x.ranks()) >= d:
        if iterations >= max_iterations:
            return None, iterations, widest, f"stopped after {iterations} iterations"
        need = square_bytes(x, pre_qc_rank)
        if need > max_bytes:
            return None, iterations, widest, (f"stopped before iteration {iterations + 1}: ranks up to {max(x.ranks())} enter "
                                              f"the square, pre-QC rank {pre_qc_rank(max(x.ranks()))}, cores of {need / 2**30:.1f} GiB")
        t0 = time.perf_counter()
        iterations += 1
        entering = pre_qc_rank(max(x.ranks()))
        widest = max(widest, entering)
        x = square(x)
        x.soft_threshold(tau, True)
        xn = max(x[rank_one_estimate(x)], (1 - (1 - alpha) * alpha / 2.0) * xn * xn)
        f_norm = x.frob_norm()
        if not (f_norm > 0.0 and f_norm < float("inf")):
            raise RuntimeError("the norm of the iterate is zero or not finite")
        xn /= f_norm
        x = x / f_norm
        tau = (1 - alpha) * alpha * xn * xn / (2.0 * (d - 1))
        if log:
            print(f"    {log} iteration {iterations}: pre-QC rank {entering}, largest rank after the threshold {max(x.ranks())}, "
                  f"{(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
    return xe.find_largest_entry(x, 0.0, 0.0), iterations, widest, None


def timed(fn):
    xe.synchronize()
    t0 = time.perf_counter()
    out = fn()
    xe.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return f"median {statistics.median(ms):10.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}, {len(ms)} runs)"


def probe(order, n, rank, reps, max_bytes):
    xe.seed(1000 * n + rank)
    t = xe.TTTensor.random([n] * order, [rank] * (order - 1))
    t = t / t.frob_norm()
    lower_bound = abs(t[rank_one_estimate(t)])
    print(f"order {order}, mode size {n}, ranks {t.ranks()}, accuracy {ACCURACY}, lowerBound {lower_bound:.6e}", flush=True)
    sym = (xe.entrywise_square, lambda r: r * (r + 1) // 2)
    kro = (lambda x: xe.entrywise_product(x, x), lambda r: r * r)

    def run(variant, limit=1000, log=None):
        return loop(t, ACCURACY, lower_bound, variant[0], variant[1], max_bytes, limit, log)

    # untimed replays: iteration counts and ranks, and the warm-up of both variants
    try:
        pos_a, it_a, wide_a, note_a = run(sym, log="(a)")
        pos_b, it_b, wide_b, note_b = run(kro, log="(b)")
    except (RuntimeError, MemoryError) as e:
        print(f"  failed: {str(e).splitlines()[0][:200]}", flush=True)
        return
    for name, note in (("(a)", note_a), ("(b)", note_b)):
        if note:
            print(f"  {name} {note}", flush=True)
    complete = note_a is None and note_b is None
    k = min(it_a, it_b)
    if not complete and k == 0:
        return
    if complete:
        first = lambda: xe.find_largest_entry(t, ACCURACY, lower_bound)  # noqa: E731
        second = lambda: run(kro)[0]  # noqa: E731
        first()
    else:
        print(f"  timing the first {k} iteration(s) of both loops", flush=True)
        wide_a, wide_b = run(sym, k)[2], run(kro, k)[2]
        first = lambda: run(sym, k)[0]  # noqa: E731
        second = lambda: run(kro, k)[0]  # noqa: E731
    ta, tb = [], []
    for rep in range(reps):
        ms, got_a = timed(first)
        ta.append(ms)
        ms, got_b = timed(second)
        tb.append(ms)
        print(f"  run {rep + 1}: (a) {ta[-1]:.2f} ms, (b) {tb[-1]:.2f} ms", flush=True)
    print(f"  (a) symmetric square : {summary(ta)}; {it_a if complete else k} iterations, largest pre-QC rank {wide_a}"
          + (f", position {got_a}" if complete else ""))
    print(f"  (b) Kronecker square : {summary(tb)}; {it_b if complete else k} iterations, largest pre-QC rank {wide_b}"
          + (f", position {got_b}" if complete else ""))
    print(f"  (b) / (a) = {statistics.median(tb) / statistics.median(ta):.2f}"
          + (f"; positions {'agree' if got_a == got_b == pos_a == pos_b else 'DIFFER'}" if complete else ""), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2x8,3x16,4x24")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--order", type=int, default=16)
    ap.add_argument("--max-gib", type=float, default=8.0)
    a = ap.parse_args()
    for size in a.sizes.split(","):
        n, rank = (int(v) for v in size.split("x"))
        probe(a.order, n, rank, a.reps, a.max_gib * 2**30)


if __name__ == "__main__":
    main()
