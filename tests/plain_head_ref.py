"""TEST INFRASTRUCTURE ONLY -- fp64 CPU restatement of the two plain-head models, composed from oracle.jspsr_ref:

* JSPSR(spn=False): the JSPSR trunk up to conv0, then postprocessor = Basic2d(2 nf, 1, 3, bn=False, relu=False)
  (reference models/JSPSR.py:195-204,378);
* EDSR(scale=1, spn=False): entry, residual trunk, tail, then head = nn.Conv2d(n_features, 1, 3, padding=1)
  (models/EDSR.py:108-111,123-136).

Every convolution / ReLU goes through ``R.F`` (the module attribute), so tests/fixtures.py's noise-floor and kink-census
stand-ins, which swap ``R.F``, see them.  Pinned by tests/golden/g9_*.npz (tools/gen_golden_plain.py).
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch

from oracle import jspsr_ref as R


def jspsr_plain_param_shapes(in_channels: dict, num_feature=32, layers=(2, 2, 2, 2)) -> Dict[str, tuple]:
    """State-dict shapes of models.JSPSR.Model(spn=False), in the reference's order."""
    out = {k: v for k, v in R.jspsr_param_shapes(in_channels, num_feature, layers).items()
           if not k.startswith(("generator.", "postprocessor."))}
    out["postprocessor.conv.0.weight"] = (1, 2 * num_feature, 3, 3)
    out["postprocessor.conv.0.bias"] = (1,)
    return out


def jspsr_trunk(c: R.Ctx, inputs: Sequence[torch.Tensor], layers=(2, 2, 2, 2)):
    """JSPSR.py:208-369: the branches, the four fused stages and the decoder -> c0 (B, 2 nf, H, W)."""
    sd = c.sd
    has_img = "conv_img.conv.0.weight" in sd
    has_aux = "conv_aux.conv.0.weight" in sd
    if len(inputs) != 1 + int(has_img) + int(has_aux):
        raise NotImplementedError
    feats = {"dem": R.basic2d(c, inputs[0], "conv_dem", 5, bn=False)}
    if has_img:
        feats["img"] = R.basic2d(c, inputs[1], "conv_img", 5, bn=True)
    if has_aux:
        feats["aux"] = R.basic2d(c, inputs[-1], "conv_aux", 5, bn=False)
    order = [k for k in ("dem", "img", "aux") if k in feats]
    fuse = []
    for stage in range(4):
        nxt = {}
        for br in order:
            src = fuse[-1] if (br == "dem" and stage > 0) else feats[br]
            nxt[br] = R.layer(c, src, f"layer{stage + 1}_{br}", layers[stage], 1 if stage == 0 else 2)
        feats = nxt
        fuse.append(torch.cat([feats[b] for b in order], 1))
    x = fuse[3]
    for name, skip in (("layer3d", fuse[2]), ("layer2d", fuse[1]), ("layer1d", fuse[0])):
        x = torch.cat((R.basic2d_trans(c, x, name), skip), 1)
    return R.basic2d(c, x, "conv0", 3, bn=True, relu=True, camb=True)


def jspsr_plain_forward(sd, inputs, training: bool, layers=(2, 2, 2, 2), return_c0=False):
    """models.JSPSR.Model(spn=False).forward."""
    c = R.Ctx(sd, training)
    c0 = jspsr_trunk(c, inputs, layers)
    out = R.basic2d(c, c0, "postprocessor", 3, bn=False, relu=False)
    return (out, c0) if return_c0 else out


def edsr_plain_param_shapes(in_channels: int, n_resblocks=16, n_features=64) -> Dict[str, tuple]:
    out = {k: v for k, v in R.edsr_param_shapes(in_channels, n_resblocks, n_features).items()
           if k.startswith(("entry.", "encoder."))}
    out["head.weight"] = (1, n_features, 3, 3)
    out["head.bias"] = (1,)
    return out


def edsr_plain_forward(sd, x: torch.Tensor, training: bool, n_resblocks=16, res_scale=0.1):
    """models.EDSR.EDSR(scale=1, spn=False).forward (EDSR.py:123-136); x = cat(dem, guides)."""
    xs = R.F.conv2d(x, sd["entry.weight"], sd["entry.bias"], 1, 1)
    h = xs
    for i in range(n_resblocks):  # ResBlock.forward, EDSR.py:40-44
        r = R.F.conv2d(h, sd[f"encoder.{i}.body.0.weight"], sd[f"encoder.{i}.body.0.bias"], 1, 1)
        r = R.F.conv2d(R.F.relu(r), sd[f"encoder.{i}.body.2.weight"], sd[f"encoder.{i}.body.2.bias"], 1, 1)
        h = r * res_scale + h
    h = R.F.conv2d(h, sd[f"encoder.{n_resblocks}.weight"], sd[f"encoder.{n_resblocks}.bias"], 1, 1)
    h = h + res_scale * xs
    return R.F.conv2d(h, sd["head.weight"], sd["head.bias"], 1, 1)
