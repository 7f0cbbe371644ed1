"""The eigensolver suite's inputs (tests/syev_spectra.py) judged without a GPU: on every case that
tests/test_syev_gpu.py runs, LAPACK's own eigenpairs meet that file's bars (so a failure there is the kernel's),
the case has the clusters it claims, and the cut lies in a gap > 1e-3 ||A|| wherever projectors are compared."""
import numpy as np
import pytest

import syev_spectra as sp


@pytest.fixture(scope="module")
def solved():
    cache = {}

    def get(gen_id, gen):
        if gen_id not in cache:
            A, meta = gen()
            w, Z = np.linalg.eigh(A)
            cache[gen_id] = (A, meta, w[::-1].copy(), Z[:, ::-1].copy())
        return cache[gen_id]
    return get


@pytest.mark.parametrize("cid,family,gen,kk", sp.CASES, ids=sp.IDS)
def test_reference_meets_the_bars(solved, cid, family, gen, kk):
    A, meta, w, Z = solved(cid.rsplit("-kk", 1)[0], gen)
    n = A.shape[0]
    assert np.array_equal(A, A.T) and 2 <= n <= 256 and 1 <= kk <= n
    nrm = np.linalg.norm(A, 2)
    spec = meta["spec"]
    assert np.abs(np.abs(spec).max() - nrm) <= 1e-13 * nrm
    lam, U = w[:kk], Z[:, :kk]
    assert np.abs(lam - spec[:kk]).max() <= 1e-13 * nrm
    assert np.abs(U.T @ U - np.eye(kk)).max() <= 1e-12
    assert np.linalg.norm(A @ U - U * lam, axis=0).max() <= 1e-12 * nrm
    # the claimed clusters: members within tol ||A|| (+ LAPACK's own 1e-13 ||A||), the neighbours outside
    # further than the solver's cluster threshold 1e-3 ||A||
    for first, members in meta["clusters"]:
        assert w[first] - w[first + members - 1] <= (meta["tol"] + 1e-13) * nrm
        if first > 0:
            assert w[first - 1] - w[first] > 1e-3 * nrm
        if first + members < n:
            assert w[first + members - 1] - w[first + members] > 1e-3 * nrm
    if sp.projector_unique(meta, kk):
        assert w[kk - 1] - w[kk] > 1e-3 * nrm


def test_case_list_covers_the_families():
    fams = {c[1] for c in sp.CASES}
    assert fams == set("abcdefgh") and len(set(sp.IDS)) == len(sp.IDS)
    a = [c for c in sp.CASES if c[1] == "a"]
    assert len(a) == 8 * 3 * 2 + 1
    # the sweep crosses the start vectors' former period (17) and the bidiagonal SVD's cluster limit (24)
    assert {int(c[0].split("-")[1][1:]) for c in a if c[0].startswith("a-m")} == {16, 17, 18, 20, 24, 25, 34, 40}


@pytest.mark.parametrize("mult", [16, 25, 40])
@pytest.mark.parametrize("layout", ["top", "middle", "straddle"])
def test_cluster_layouts(mult, layout):
    kk = mult + 10
    A, meta = sp.cluster(96, mult, layout, 0.0, 1, kk)
    (first, members), = meta["clusters"]
    assert members == mult
    s = meta["spec"]
    gaps = -np.diff(s)
    distinct = np.delete(gaps, np.arange(first, first + mult - 1))
    assert distinct.min() > 1e-2 * s[0]
    if layout == "top":
        assert first == 0 and sp.projector_unique(meta, kk)
    elif layout == "middle":
        assert 0 < first and first + mult < kk and sp.projector_unique(meta, kk)
    else:
        assert first < kk < first + mult and not sp.projector_unique(meta, kk)
