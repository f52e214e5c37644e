"""CPU tests of the ADM UNet options' boundary (use_scale_shift_norm, resblock_updown, conv_resample=False,
num_classes, conditioning_key='adm'): construction, state_dict keys against the reference's
(tests/golden/make_golden_adm.py), argument validation, and the new C ABI symbols in the header / binding /
library / INTEGRATION.md."""
import json
import os
import re

import pytest
import torch

import adm_util as au
from golden_util import cfg_of, load, weights_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sdk_group_norm_film", "sdk_group_norm_resample", "sdk_embedding_add")


def _unet(sdk, cfg):
    from sd_amd.openai_model.model import UNetModel
    return UNetModel(**cfg)


@pytest.mark.parametrize("name", list(au.FIXTURES))
def test_constructs_with_the_reference_state_dict_keys(sdk, name):
    cfg, seed = au.FIXTURES[name]
    z = load(name)
    assert cfg_of(z) == cfg and int(z["seed"]) == seed
    m = _unet(sdk, cfg)
    ref = [(k, tuple(s)) for k, s in json.loads(bytes(z["keys"]).decode())]
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == ref                                    # names, shapes and order
    assert not [k for k, _ in got if ".h_upd." in k or ".x_upd." in k]
    m.load_state_dict(weights_of(z))                     # strict


def test_class_head_film_rows_and_resampling_blocks(sdk):
    from sd_amd.openai_model.model import Downsample, ResBlock, Upsample
    m = _unet(sdk, au.ADM_FULL)
    sd = m.state_dict()
    te = 4 * au.ADM_FULL["model_channels"]
    assert tuple(sd["label_emb.weight"].shape) == (10, te)
    assert list(sd)[4] == "label_emb.weight"             # right after time_embed, as the reference registers it
    for name, rb in m.named_modules():
        if isinstance(rb, ResBlock):
            assert tuple(sd[name + ".emb_layers.1.weight"].shape) == (2 * rb.out_channels, te), name
    down = [rb for rb in m.modules() if isinstance(rb, ResBlock) and isinstance(rb.h_upd, Downsample)]
    up = [rb for rb in m.modules() if isinstance(rb, ResBlock) and isinstance(rb.h_upd, Upsample)]
    assert len(down) == 2 and len(up) == 2               # one per level transition, each way
    for rb in down + up:
        assert rb.updown and not list(rb.h_upd.parameters()) and not list(rb.x_upd.parameters())
        assert not rb.h_upd.use_conv and isinstance(rb.skip_connection, torch.nn.Identity)
    # no stand-alone resampling layers are left in the block lists
    assert not [l for blk in list(m.input_blocks) + list(m.output_blocks) for l in blk
                if isinstance(l, (Downsample, Upsample))]
    pool = _unet(sdk, au.ADM_POOL)
    assert [type(l.op).__name__ for blk in pool.input_blocks for l in blk if isinstance(l, Downsample)] == ["AvgPool2d"]
    ups = [l for blk in pool.output_blocks for l in blk if isinstance(l, Upsample)]
    assert len(ups) == 1 and not ups[0].use_conv and not list(ups[0].parameters())


def test_all_three_skip_modes_construct_on_a_resampling_block(sdk):
    from sd_amd.openai_model.model import ResBlock
    for kw, kind in ((dict(out_channels=32), torch.nn.Identity), (dict(out_channels=64), torch.nn.Conv2d),
                     (dict(out_channels=64, use_conv=True), torch.nn.Conv2d)):
        for d in (dict(up=True), dict(down=True)):
            rb = ResBlock(32, 128, 0.0, use_scale_shift_norm=True, **kw, **d)
            assert isinstance(rb.skip_connection, kind)
            assert rb.emb_layers[1].out_features == 2 * rb.out_channels
    assert ResBlock(32, 128, 0.0, out_channels=64, use_conv=True, down=True).skip_connection.kernel_size == (3, 3)


def test_still_refused_options_raise(sdk):
    with pytest.raises(NotImplementedError, match="n_embed"):
        _unet(sdk, dict(au.ADM_FULL, n_embed=64))
    with pytest.raises(NotImplementedError, match="dims"):
        _unet(sdk, dict(au.ADM_POOL, dims=3))
    from sd_amd.openai_model.utils import timestep_embedding
    with pytest.raises(NotImplementedError, match="repeat_only"):
        timestep_embedding(torch.zeros(2, dtype=torch.long), 32, repeat_only=True)


def test_forward_takes_y_iff_class_conditional(sdk):
    x, t, ctx = torch.zeros(2, 4, 16, 16), torch.zeros(2, dtype=torch.long), torch.zeros(2, 7, 48)
    with pytest.raises(AssertionError, match="class-conditional"):
        _unet(sdk, au.ADM_FULL)(x, t, context=ctx)                            # y missing
    with pytest.raises(AssertionError, match="class-conditional"):
        _unet(sdk, au.ADM_FILM_ONLY)(x, t, context=ctx, y=torch.tensor([1, 2]))   # y without a class head
    with pytest.raises(AssertionError, match="shape"):
        _unet(sdk, au.ADM_FULL)(x, t, context=ctx, y=torch.tensor([1, 2, 3]))


@pytest.mark.parametrize("bad", [[3, 10], [-1, 2]])
def test_host_label_out_of_range_raises_index_error(sdk, bad):
    m = _unet(sdk, au.ADM_FULL)
    x, t, ctx = torch.zeros(2, 4, 16, 16), torch.zeros(2, dtype=torch.long), torch.zeros(2, 7, 48)
    with pytest.raises(IndexError, match="out of range"):
        m(x, t, context=ctx, y=torch.tensor(bad))


def _wrapper(sdk, unet):
    from sd_amd.Diffusion.ddpm import DiffusionWrapper
    dw = DiffusionWrapper.__new__(DiffusionWrapper)
    torch.nn.Module.__init__(dw)
    dw.diffusion_model, dw.conditioning_key, dw._graphed, dw._graphs_on = unet, "adm", None, False
    return dw


def test_adm_wrapper_needs_a_class_head_and_passes_labels_as_y(sdk):
    x, t = torch.zeros(2, 4, 16, 16), torch.zeros(2, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="class head"):
        _wrapper(sdk, _unet(sdk, au.ADM_POOL))(x, t, c_crossattn=[torch.tensor([1, 2])])
    dw = _wrapper(sdk, _unet(sdk, au.ADM_WRAP))
    with pytest.raises(ValueError, match="c_crossattn"):
        dw(x, t)
    # the labels reach UNetModel.forward as y: its host range check fires (before any device work)
    with pytest.raises(IndexError, match="out of range"):
        dw(x, t, c_crossattn=[torch.tensor([1, 10])])


def test_graph_key_holds_the_label_shape(sdk):
    from sd_amd.graphs import GraphedUNet
    x, t = torch.zeros(2, 4, 16, 16), torch.zeros(2, dtype=torch.long)
    k0 = GraphedUNet._key(x, t, None)
    k1 = GraphedUNet._key(x, t, None, (), torch.tensor([1, 2]))
    assert k0 != k1 and k1 == GraphedUNet._key(x, t, None, (), torch.tensor([7, 8]))   # by shape, not contents


def test_new_symbols_in_header_binding_library_and_integration_table(sdk):
    from sd_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sdk_amd.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = _lib.lib()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in _lib.EXPORTS, sym
        assert hasattr(L, sym), sym
        assert re.search(r"^\| `%s` \|" % sym, table, re.M), sym
    for fn in ("group_norm_film", "group_norm_resample", "embedding_add"):
        assert callable(getattr(ops, fn))
    assert (_lib.RESAMPLE_AVGPOOL2, _lib.RESAMPLE_NEAREST2) == (0, 1)
    assert re.search(r"SDK_RESAMPLE_AVGPOOL2 = 0, SDK_RESAMPLE_NEAREST2 = 1", header)
