"""CPU: the plain-head models (JSPSR spn=False, EDSR spn=False) -- fixtures made by the reference's own modules
(tests/golden/g9_*.npz, tools/gen_golden_plain.py), the fp64 restatement in tests/plain_head_ref.py, the port's
state-dict layout and init stream, and the argument checks of the K1p entry points (no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import jspsr_ref as R
from tests import fixtures as Fx
from tests import plain_head_ref as P

JSPSR_FIXTURES = [("g9_jspsr_img_nf8_b2_48x64_train.npz", Fx.IMG), ("g9_jspsr_msk_nf8_b2_64_eval.npz", Fx.MSK),
                  ("g9_jspsr_msk_nf32_b1_64_train.npz", Fx.MSK)]


def _shape_list(z):
    return [(str(k), str(s)) for k, s in zip(z["sd_keys"], z["sd_shapes"])]


@pytest.mark.parametrize("name,ic", JSPSR_FIXTURES)
def test_jspsr_plain_fixture_regenerates_and_the_oracle_matches(golden_dir, name, ic):
    z = Fx.load(golden_dir, name)
    shapes = P.jspsr_plain_param_shapes(ic, int(z["nf"]))
    sd, inputs, _ = Fx.regen(z, shapes, "mask" in ic)          # fails (never skips) if the stream moved
    assert [(k, str(v)) for k, v in shapes.items()] == _shape_list(z)
    with torch.no_grad():
        pred = P.jspsr_plain_forward(sd, inputs, bool(z["training"]))
    ref = torch.from_numpy(z["pred"])
    assert (pred - ref).abs().max().item() < 2e-5
    assert (torch.from_numpy(z["pred_fp32"]).double() - ref).abs().max().item() < 1e-4


def test_edsr_plain_fixture_regenerates_and_the_oracle_matches(golden_dir):
    z = Fx.load(golden_dir, "g9_edsr_b2_40x56_train.npz")
    n, f = int(z["n_resblocks"]), int(z["n_features"])
    shapes = P.edsr_plain_param_shapes(4, n, f)
    sd, inputs, _ = Fx.regen(z, shapes, False)
    assert [(k, str(v)) for k, v in shapes.items()] == _shape_list(z)
    with torch.no_grad():
        pred = P.edsr_plain_forward(sd, torch.cat(inputs, 1), True, n)
    assert (pred - torch.from_numpy(z["pred"])).abs().max().item() < 2e-5


def test_oracle_gradients_match_the_reference_made_gradients(golden_dir):
    """The helper's autograd reproduces the reference modules' stored gradients (head and the layers feeding it)."""
    z = Fx.load(golden_dir, "g9_jspsr_img_nf8_b2_48x64_train.npz")
    sd, inputs, _ = Fx.regen(z, P.jspsr_plain_param_shapes(Fx.IMG, 8), False)
    probe = R.probe_gradient(tuple(z["pred"].shape), int(z["seed"]) + 2)
    _, g = Fx.oracle_gradients(lambda s, i: P.jspsr_plain_forward(s, i, True), sd, inputs, probe)
    keys = [k[5:] for k in z.files if k.startswith("grad:")]
    assert "postprocessor.conv.0.weight" in keys and "conv0.conv.0.weight" in keys
    for k in keys:
        assert Fx.rel(g[k], z["grad:" + k]) < 1e-9, k
    assert [str(k) for k in z["grad_names"]] == list(g)


@pytest.mark.parametrize("name,ic", JSPSR_FIXTURES)
def test_port_jspsr_plain_state_dict_is_the_reference_layout(golden_dir, name, ic):
    from jspsr_amd.JSPSR import Model
    z = Fx.load(golden_dir, name)
    m = Model(dict(ic, COP30=1), num_feature=int(z["nf"]), spn=False)
    assert [(k, str(tuple(v.shape))) for k, v in m.state_dict().items()] == _shape_list(z)
    assert m.generator is None and m.receptive_radius == 92 and m.learned_offsets is False


def test_port_edsr_plain_state_dict_is_the_reference_layout(golden_dir):
    from jspsr_amd.EDSR import EDSR
    z = Fx.load(golden_dir, "g9_edsr_b2_40x56_train.npz")
    m = EDSR(in_channels=4, out_channels=1, n_resblocks=4, n_features=32, scale=1)     # spn unset: the reference default
    assert [(k, str(tuple(v.shape))) for k, v in m.state_dict().items()] == _shape_list(z)
    assert m.receptive_radius == 2 * 4 + 3 and m.learned_offsets is False
    assert EDSR.receptive_radius is None and not hasattr(EDSR(4, 1, 2, 16, 1, spn=True), "learned_offsets")


def test_port_init_stream_equals_reference(golden_dir):
    from jspsr_amd.JSPSR import Model
    z = Fx.load(golden_dir, "g9_init_stream_msk_nf8.npz")
    np.random.seed(int(z["seed"]))
    sd = Model(dict(Fx.MSK, COP30=1), num_feature=int(z["nf"]), spn=False).state_dict()
    assert list(sd) == [str(k) for k in z["names"]]
    for i, k in enumerate(sd):
        t = sd[k].double().reshape(-1)
        got = np.array([t.sum().item(), t.abs().sum().item(), t[0].item(), t[-1].item()])
        assert np.array_equal(got[2:], z["summary"][i][2:]), k
        assert np.allclose(got[:2], z["summary"][i][:2], rtol=0, atol=1e-12 * got[1]), k


def test_unbuilt_configurations_still_raise():
    from jspsr_amd.EDSR import EDSR
    from jspsr_amd.JSPSR import Model
    with pytest.raises(NotImplementedError):
        Model(dict(Fx.IMG, COP30=1), out_channels=2, num_feature=8, spn=False)
    with pytest.raises(NotImplementedError):
        EDSR(in_channels=4, out_channels=1, n_resblocks=2, n_features=16, scale=2)
    with pytest.raises(NotImplementedError):
        EDSR(in_channels=4, out_channels=3, n_resblocks=2, n_features=16, scale=1)


def test_head1_entry_points_validate_arguments_without_a_gpu():
    from jspsr_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)          # never dereferenced: every check below fails before a launch
    assert lib.jspsr_conv_head1_forward(0, None, 64, 0, 64, fake, fake, fake, 1, 8, 8, None) == -1
    assert b"null" in lib.jspsr_last_error()
    assert lib.jspsr_conv_head1_backward(1, fake, fake, 64, 0, 64, None, None, 64, 0, fake, fake, fake, 1, 8, 8, None) == -1
    for C in (12, 264, 0, -8):
        assert lib.jspsr_conv_head1_forward(1, fake, 512, 0, C, fake, fake, fake, 1, 8, 8, None) == -1, C
        assert b"C = " in lib.jspsr_last_error()
        assert lib.jspsr_conv_head1_backward(0, fake, fake, 512, 0, C, fake, None, 512, 0, fake, fake, fake, 1, 8, 8, None) == -1
        assert lib.jspsr_conv_head1_workspace_bytes(1, 8, 8, C) == 0
    assert lib.jspsr_conv_head1_forward(2, fake, 64, 0, 64, fake, fake, fake, 1, 8, 8, None) == -1        # dtype
    assert lib.jspsr_conv_head1_forward(1, fake, 60, 0, 64, fake, fake, fake, 1, 8, 8, None) == -1        # pitch < C
    assert lib.jspsr_conv_head1_forward(1, fake, 72, 4, 64, fake, fake, fake, 1, 8, 8, None) == -1        # bf16 offset 4
    assert lib.jspsr_conv_head1_forward(0, fake, 64, 0, 64, fake, fake, fake, 0, 8, 8, None) == -1        # B = 0


def test_head1_workspace_formula():
    from jspsr_amd import _lib
    lib = _lib.load()
    for B, H, W, C in ((8, 512, 512, 64), (1, 1, 1, 8), (2, 37, 61, 256), (3, 65, 129, 24)):
        tiles = B * -(-H // 32) * -(-W // 64)
        assert lib.jspsr_conv_head1_workspace_bytes(B, H, W, C) == tiles * (9 * C + 1) * 4
    assert lib.jspsr_conv_head1_workspace_bytes(0, 8, 8, 8) == 0
