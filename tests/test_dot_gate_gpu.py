"""Where a gated asynchronous <x,y> starts beside a round (csrc/tt.hip: open_dot_gate). In the two-chain pass of an
unsharded certified round the gate opens behind the last full-size step of the interleaved Gram chains (dot_gate_step),
or one full-size step earlier (the default), so the product's first steps run beside the chains' thin tail; every
other path opens it where it did before. The
product reads the pre-round cores, which the round releases only behind it: its value must be bit for bit the
synchronous product of the pre-round tensor, and the round's cores byte for byte those of a round alone, wherever the
gate opens (XRS_DOT_GATE_EARLY = 0: behind the chains, e >= 1: behind the e-th full-size step from the end, 2 the
default; read at every pass)."""
import numpy as np
import pytest

from xerus_amd import capi

pytestmark = pytest.mark.gpu

# name: (dims, ranks, rank bound of the round, must the round take the certified chain path). "no_thin_step" has raw
# Gaussian cores of rank 4 on modes of 3 (its outer edges are rank deficient: the certificate refuses them; the
# oracle's generators would cut those ranks to 3).
TRAINS = {
    "thin_ends_full_middle": ([4] * 6, [4, 16, 16, 16, 4], 16, True),
    "no_thin_step": ([3] * 4, [4, 4, 4], 4, False),
    "d2": ([5, 6], [4], 4, False),
    "d3": ([7, 3, 5], [6, 4], 6, False),
    "truncating": ([4] * 6, [4, 16, 16, 16, 4], 8, False),
}


def _same_bytes(a_cores, b_cores):
    return len(a_cores) == len(b_cores) and all(a.shape == b.shape and a.tobytes() == b.tobytes()
                                                for a, b in zip(a_cores, b_cores))


def _pair(ref, name):
    """The cores of x and y."""
    dims, ranks, _, _ = TRAINS[name]
    if name == "no_thin_step":
        rng = np.random.default_rng(7)
        r = [1] + ranks + [1]
        return tuple([rng.standard_normal((r[k], dims[k], r[k + 1])) for k in range(len(dims))] for _ in range(2))
    x, y = ref.TT.random(dims, ranks, ref.Rng(7)), ref.TT.random(dims, ranks, ref.Rng(43))
    assert x.ranks == ranks
    return x.cores, y.cores


def _full(cores):
    t = cores[0]
    for c in cores[1:]:
        t = np.tensordot(t, c, axes=([t.ndim - 1], [0]))
    return t.ravel()


@pytest.mark.parametrize("early", ("default", "0", "1", "2", "3"))
@pytest.mark.parametrize("name", list(TRAINS))
def test_dot_async_beside_round_is_the_synchronous_product(handle, ref, monkeypatch, name, early):
    xc, yc = _pair(ref, name)
    _, _, bound, chain = TRAINS[name]
    gy = capi.TTDevice.from_cores(handle, yc)
    alone = capi.TTDevice.from_cores(handle, [c.copy() for c in xc])
    d_sync = alone.dot(gy)
    fx, fy = _full(xc), _full(yc)
    assert abs(d_sync - fx @ fy) <= 1e-12 * np.linalg.norm(fx) * np.linalg.norm(fy)
    alone.round(bound)
    path = handle.last_round_path()
    if chain:
        assert path == "chain"
    expect = alone.cores()
    alone.free()
    if early == "default":
        monkeypatch.delenv("XRS_DOT_GATE_EARLY", raising=False)
    else:
        monkeypatch.setenv("XRS_DOT_GATE_EARLY", early)
    for i in range(3):
        g = capi.TTDevice.from_cores(handle, [c.copy() for c in xc])
        fut = g.dot_async(gy)
        g.round(bound)
        d = fut.result()
        assert handle.last_round_path() == path
        out = g.cores()
        g.free()
        assert d == d_sync, (name, early, i, d, d_sync)
        assert _same_bytes(out, expect), (name, early, i)
    gy.free()


@pytest.mark.parametrize("name", ("thin_ends_full_middle", "d2", "d3"))
def test_dot_async_with_no_round_behind_it(handle, ref, name):
    """Nothing opens the gate but the wait itself."""
    xc, yc = _pair(ref, name)
    gx, gy = capi.TTDevice.from_cores(handle, xc), capi.TTDevice.from_cores(handle, yc)
    d_sync = gx.dot(gy)
    for i in range(3):
        assert gx.dot_async(gy).result() == d_sync, (name, i)
    gx.free()
    gy.free()
