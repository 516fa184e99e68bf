"""The chip-wide gate MLP kernels (gate_mlp_hidden / gate_mlp_out, gate_mlp_bwd_hidden / gate_mlp_bwd_in) against the
one-workgroup-per-image kernels they replaced, which stay reachable through jspsr_gate_mlp_legacy: every sum keeps its
order of operations, so forward (s, hid) and backward (davg, dmax, dw1, dw2) must agree bit for bit -- torch.equal, no
tolerance.  (test_elementwise_gpu.test_gate_mlp_kernels_against_torch_autograd checks the values themselves.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

NEW = ("gate_mlp_hidden", "gate_mlp_out", "gate_mlp_bwd_hidden", "gate_mlp_bwd_in")
OLD = ("gate_mlp_forward", "gate_mlp_backward")


def _counts():
    from jspsr_amd import _lib
    lib = _lib.load()
    return {n: lib.jspsr_launch_count(n.encode()) for n in NEW + OLD}


def _run(K, t):
    s, hid = K.gate_mlp_forward(t["avg"], t["mx"], t["w1"], t["w2"])
    davg, dmax, dw1, dw2 = K.gate_mlp_backward(t["ds"], s, hid, t["avg"], t["mx"], t["w1"], t["w2"])
    torch.cuda.synchronize()
    return dict(s=s, hid=hid, davg=davg, dmax=dmax, dw1=dw1, dw2=dw2)


@pytest.mark.parametrize("B,C,Ch", [
    (1, 16, 1),
    (3, 64, 4),
    (2, 200, 12),      # C is not a multiple of 64
    (2, 72, 9),        # Ch is not a multiple of the wave count, nor of the four hidden units a backward wave takes
    (8, 1536, 96),     # the training step's widest gate
])
def test_wide_gate_mlp_equals_legacy_bit_for_bit(B, C, Ch):
    from jspsr_amd import kernels as K
    g = torch.Generator().manual_seed(1000 * B + C + Ch)
    r = lambda *shape, k=1.0: (k * torch.randn(*shape, generator=g)).cuda()
    # weights large enough that ReLUs close, the sigmoid leaves its linear part and the images' s differ
    t = dict(avg=r(B, C), mx=r(B, C, k=2.0), w1=r(Ch, C, k=3.0 / C ** 0.5), w2=r(C, Ch, k=2.0 / Ch ** 0.5), ds=r(B, C))
    prev = K.gate_mlp_legacy(-1)
    try:
        K.gate_mlp_legacy(0)
        c0 = _counts()
        new = _run(K, t)
        c1 = _counts()
        K.gate_mlp_legacy(1)
        old = _run(K, t)
        c2 = _counts()
    finally:
        K.gate_mlp_legacy(int(prev))
    assert all(c1[n] == c0[n] + 1 for n in NEW) and all(c1[n] == c0[n] for n in OLD), (c0, c1)
    assert all(c2[n] == c1[n] + 1 for n in OLD) and all(c2[n] == c1[n] for n in NEW), (c1, c2)
    hid = old["hid"]
    assert 0 < (hid == 0).sum().item() < hid.numel() or Ch == 1, "the case should close some ReLUs and open others"
    for k in ("s", "hid", "davg", "dmax", "dw1", "dw2"):
        assert torch.isfinite(old[k]).all(), k
        assert torch.equal(new[k], old[k]), (k, (new[k] - old[k]).abs().max().item())
