"""Generates tests/golden/oracle_check/*.npz: the REAL reference's outputs for the small ViT-S cases of tests/test_oracle_vs_reference.py, so that
the oracle is held to the reference tensor for tensor on every machine, not only where the reference tree can be imported.

    ADA_REFERENCE_ROOT=<reference checkout> python oracle/make_golden_oracle_check.py

Each fixture stores the reference model's state_dict schema (ordered keys, shapes, dtypes -- the test fills it with fill_state_dict_, whose draws
depend on the key and the seed only), the reference output, and for the raw model its input (drawn here from a fixed seed).  The amodal inputs
are make_inputs(2, 98, 126, 4), rebuilt by the test.  Both forwards run in float64 (parameters and inputs; the fill is drawn in fp32 first): in fp32
the last bits of a forward follow the CPU's kernels and thread count, so a stored fp32 output could not be matched to 1e-6 on another machine.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "amodal-depth-anything_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import _refshim  # noqa: E402
from oracle import dav2_oracle as O  # noqa: E402
from src.util.synth_weights import fill_state_dict_, make_inputs  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "oracle_check")
AMODAL_CASES = [("mask+observation", "entire_target_object"), ("image+mask+observation", "x_ssi"), ("none", "y")]
AMODAL_WEIGHT_SEED, AMODAL_INPUTS = 3, (2, 98, 126, 4)
RAW = dict(encoder="vits", features=64, out_channels=[48, 96, 192, 384], weight_seed=5, input_shape=[1, 3, 70, 112], input_seed=7)


def amodal_name(guide_type, loss):
    return "amodal_vits_" + guide_type.replace("+", "_") + "_" + loss


def _schema(sd):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]


def _f64(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def _save(name, out, meta, **arrays):
    os.makedirs(OUT_DIR, exist_ok=True)
    np.savez_compressed(os.path.join(OUT_DIR, name + ".npz"), out=out.numpy(), meta=np.array(json.dumps(meta)), **arrays)
    print(name, tuple(out.shape), "max |oracle - reference| =", meta["oracle_vs_reference_maxabs"])


def main():
    Amodal, Raw = _refshim.load_reference()
    for guide_type, loss in AMODAL_CASES:
        m = Amodal(guide_type=guide_type, loss_stategy=loss, encoder="vits", pretrained=False).eval()
        sd = m.state_dict()
        fill_state_dict_(sd, AMODAL_WEIGHT_SEED)
        m.load_state_dict(sd, strict=True)
        m, sd = m.double(), _f64(sd)
        x, grgb, mask, obs = (t.double() for t in make_inputs(*AMODAL_INPUTS))
        with torch.no_grad():
            ref = m(x, guide_rgb=grgb, guide_mask=mask, observation=obs)
        mine = O.amodal_forward(sd, "vits", guide_type, loss, x, grgb, mask, obs)
        meta = {"guide_type": guide_type, "loss": loss, "encoder": "vits", "weight_seed": AMODAL_WEIGHT_SEED, "inputs": list(AMODAL_INPUTS),
                "schema": _schema(sd), "oracle_vs_reference_maxabs": float((mine - ref).abs().max())}
        _save(amodal_name(guide_type, loss), ref, meta)
    m = Raw(encoder=RAW["encoder"], features=RAW["features"], out_channels=RAW["out_channels"]).eval()
    sd = m.state_dict()
    fill_state_dict_(sd, RAW["weight_seed"])
    m.load_state_dict(sd, strict=True)
    m, sd = m.double(), _f64(sd)
    x = torch.randn(*RAW["input_shape"], generator=torch.Generator().manual_seed(RAW["input_seed"])).double()
    with torch.no_grad():
        ref = m(x)
    mine = O.raw_forward(sd, RAW["encoder"], x)
    meta = dict(RAW, schema=_schema(sd), oracle_vs_reference_maxabs=float((mine - ref).abs().max()))
    _save("raw_vits", ref, meta, x=x.numpy())


if __name__ == "__main__":
    main()
