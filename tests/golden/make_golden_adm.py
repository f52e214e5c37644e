"""Generate the ADM-option UNet fixtures by running the REFERENCE itself (build container only, CPU).

Run from the repo root:  python tests/golden/make_golden_adm.py
Needs the reference checkout make_golden.py points at (read-only) and einops.  Uses the shims of make_golden.py
(flash_attn / omegaconf / Lightning / torchvision stand-ins, identity ``.half()``).

The reference's own ``openai_model.model.UNetModel`` is built for each configuration of tests/adm_util.py
(use_scale_shift_norm, resblock_updown, conv_resample=False, num_classes), its weights replaced by
``make_golden.reinit_`` (tests/golden/synth.py: regenerated in the tests, not stored; the zero-initialised convs
become non-zero), and run in fp32 on inputs regenerated from seeds (adm_util.inputs).  The 'adm' case goes through
the reference's ``DiffusionWrapper.forward`` (``Diffusion/ddpm.py:65-67``) on a stand-in ``self``.

* unet_tiny_adm_full.npz — ADM_FULL on the 16x16 input (``y``) and on the 8x24 one (``y_wide``);
* unet_tiny_adm_pool.npz — ADM_POOL (avg-pool Downsample, conv-less Upsample);
* unet_tiny_adm_film.npz — ADM_FILM_ONLY;
* unet_tiny_adm_wrap.npz — ADM_WRAP through DiffusionWrapper.forward(conditional_key='adm', c_crossattn=[y]).

Each holds ``keys`` (state_dict key order + shapes), ``cfg``, ``seed`` and the outputs.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                    # noqa: E402
import adm_util as au                                       # noqa: E402

OUT = HERE
T = torch.from_numpy


def build(name):
    cfg, seed = au.FIXTURES[name]
    with mg.quiet():
        from openai_model.model import UNetModel
        torch.manual_seed(seed)
        m = UNetModel(**cfg)
    mg.reinit_(m, seed)
    m.eval()
    out = dict(mg.sd_keys(m), seed=np.int64(seed), cfg=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8))
    return m, out


def save(name, out):
    for k, v in out.items():
        if k.startswith("y"):
            assert np.isfinite(v).all() and np.abs(v).max() > 1e-3, f"{name}/{k}: degenerate output"
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)


def gen_full():
    m, out = build("unet_tiny_adm_full")
    for key, shape in (("y", (2, 4, 16, 16)), ("y_wide", au.WIDE)):
        d = {k: T(v) for k, v in au.inputs(shape).items()}
        with mg.quiet(), torch.no_grad():
            out[key] = m(d["x"], d["t"], context=d["ctx"], y=d["y"]).numpy()
            other = m(d["x"], d["t"], context=d["ctx"], y=(d["y"] + 1) % 10).numpy()
        # the label must matter, else a missing label add could pass
        assert np.abs(out[key] - other).max() > 1e-3 * np.abs(out[key]).max(), "labels do not reach the output"
    save("unet_tiny_adm_full", out)


def gen_plain(name, with_ctx):
    m, out = build(name)
    d = {k: T(v) for k, v in au.inputs().items()}
    with mg.quiet(), torch.no_grad():
        out["y"] = m(d["x"], d["t"], context=d["ctx"] if with_ctx else None).numpy()
    save(name, out)


def gen_wrap():
    with mg.quiet():
        from Diffusion import ddpm as top
    m, out = build("unet_tiny_adm_wrap")
    d = {k: T(v) for k, v in au.inputs().items()}
    dw = types.SimpleNamespace(diffusion_model=m, conditional_key="adm")
    with mg.quiet(), torch.no_grad():
        out["y"] = top.DiffusionWrapper.forward(dw, d["x"], d["t"], c_crossattn=[d["y"]]).numpy()
        assert torch.equal(T(out["y"]), m(d["x"], d["t"], y=d["y"]))
    save("unet_tiny_adm_wrap", out)


def main():
    mg.install_shims()
    torch.set_num_threads(8)
    gen_full()
    gen_plain("unet_tiny_adm_pool", with_ctx=False)
    gen_plain("unet_tiny_adm_film", with_ctx=True)
    gen_wrap()
    for f in sorted(os.listdir(OUT)):
        if f.startswith("unet_tiny_adm") and f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
