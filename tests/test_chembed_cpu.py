"""CPU: channel embeddings of AVRModel (model.py:11-61, 71-235 of the
reference): the config rules over every reference config with a
`channel_embed` block, `InjectionMLP` against the restatement in
tests/chembed_cases.py, the kernels' argument refusals (no device call),
the tcnn state-dict layout, and the concat models' need of `ch_idx`."""
import ctypes
import os
import subprocess

import pytest
import torch

import chembed_cases as cc
from avr_amd import _lib, tcnn_compat
from avr_amd.model import MLP, AVRModel, InjectionMLP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- config rules
def _entries():
    es = [(e["file"], e["channel_embed"], e["networks"]) for e in cc.load_configs()]
    nets = es[0][2]
    # concat is in no shipped file: the ends of the optuna range of the widths
    for dim in (32, 256):
        es.append((f"synth_concat_{dim}", dict(cc.CONCAT_ALL, emb_dim_sigma_encoder=dim, emb_dim_sigma_decoder=dim,
                                               emb_dim_signal_network=dim), nets))
    es.append(("synth_concat_encoder_only", dict(cc.CONCAT_ALL, is_sigma_decoder=False, is_signal_network=False),
               nets))
    es.append(("synth_is_embed_false", dict(cc.ADD_ALL, is_embed=False), nets))
    return es


ENTRIES = _entries()


def test_fixture_covers_the_reference_configs():
    """All 111 reference configs with a `channel_embed` block, subdirectories
    included, by their path under config_files (base names repeat)."""
    files = [e["file"] for e in cc.load_configs()]
    assert len(files) == 111 and len(set(files)) == 111
    # the is_embed-without-connection_type case and the batch-8 add shape the issue names
    by = {e["file"]: e for e in cc.load_configs()}
    none = by["real_exp_ch_emb/avr_real_exp_ch_emb_24.yml"]["channel_embed"]
    assert none.get("is_embed") is True and "connection_type" not in none
    das = by["real_exp_ch_emb_add_das/avr_real_exp_ch_emb_add_das_1.yml"]
    assert das["channel_embed"]["connection_type"] == "add" and das["batch_size"] == 8
    assert (das["n_azi"], das["n_ele"], das["n_samples"]) == (64, 32, 64)
    assert "avr_real_exp_ch_emb_1.yml" in by and "real_exp_ch_emb/avr_real_exp_ch_emb_1.yml" in by
    # widths beyond the top-level files' 128 / 128 / 512 are part of the set
    widths = {tuple(e["networks"][k]["n_neurons"] for k in ("sigma_encoder_network", "sigma_decoder_network",
                                                           "signal_network")) for e in cc.load_configs()}
    assert {(256, 128, 512), (128, 64, 512), (128, 128, 1024)} <= widths
    assert os.path.getsize(cc.CONFIGS) < 100_000


@pytest.mark.parametrize("name,block,nets", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_config_rules(name, block, nets):
    cfg = cc.small_model_cfg(block)
    for k, v in nets.items():
        cfg[k] = dict(cfg[k], **v)
    torch.manual_seed(0)
    model = AVRModel(cfg)
    want = cc.expected_embedding_params(block, nets)
    assert cc.embedding_params(model) == want
    if "connection_type" not in block or not block.get("is_embed"):
        assert want == {} and not model._has_embed
    for n, p in model.named_parameters():
        if n in want:
            assert p.dtype == torch.float32 and p.requires_grad
            if p.numel():  # randn / sqrt(dim): a sample std within 20 % for >= 1024 values
                assert abs(float(p.detach().std()) / cc.embedding_init_scale(p.size(1)) - 1) < 0.2, n
    # a concat network's first layer is n_in + emb_dim wide
    if block.get("is_embed") and block.get("connection_type") == "concat":
        if block.get("is_sigma_encoder"):
            assert model._model_encoder_sigma.layers[0].weight.size(1) == 40 + block["emb_dim_sigma_encoder"]
        if block.get("is_sigma_decoder"):
            assert model._model_decoder_sigma.layers[0].weight.size(1) == 128 + block["emb_dim_sigma_decoder"]
        if block.get("is_signal_network"):
            assert model._model_signal.layers[0].weight.size(1) == 208 + block["emb_dim_signal_network"]


# ---------------------------------------------------------------- InjectionMLP
def _injection(seed=0, n_in=24, width=32, n_out=7, C=4):
    torch.manual_seed(seed)
    return InjectionMLP(n_in, n_out, dict(n_neurons=width, n_hidden_layers=3, activation="ReLU"), C)


def test_injection_mlp_matches_restatement_fp32():
    G, rows = 3, 5
    mlp = _injection()
    ch = torch.tensor([2, 0, 2])  # channel 2 twice, channels 1 and 3 unused
    x = torch.randn(G * rows, 24, requires_grad=True)
    xr = x.detach().clone().requires_grad_(True)
    out = mlp(x, ch, rows)
    ref = cc.ref_injection(xr, [l.weight for l in mlp.hidden_layers], list(mlp.layer_embeddings),
                           mlp.output_layer.weight, ch.repeat_interleave(rows), torch.float32)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-6)
    probe = torch.randn_like(out)
    params = list(mlp.parameters())
    got = torch.autograd.grad((out * probe).sum(), [x] + params)
    want = torch.autograd.grad((ref * probe).sum(), [xr] + params)
    for (n, _), a, b in zip([("x", None)] + list(mlp.named_parameters()), got, want):
        assert a.dtype == torch.float32
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")
    # unused channels get exact zeros, used ones do not
    ge = got[1 + [n for n, _ in mlp.named_parameters()].index("layer_embeddings.0")]
    assert not ge[1].any() and not ge[3].any() and ge[0].any() and ge[2].any()


def test_injection_mlp_without_index_is_the_plain_mlp():
    mlp = _injection(1)
    plain = MLP(24, 7, dict(n_neurons=32, n_hidden_layers=3, activation="ReLU"))
    with torch.no_grad():
        for a, b in zip(plain.layers, mlp.layers):
            a.weight.copy_(b.weight)
    x = torch.randn(15, 24)
    assert torch.equal(mlp(x), plain(x))
    assert torch.equal(mlp.hidden(x), plain.hidden(x))
    assert not torch.equal(mlp(x, torch.tensor([0, 1, 2]), 5), plain(x))


# ---------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "avr_amd", "csrc"), "-j8"], check=True)
    return _lib.load()


def _refused(lib, name, rc):
    assert rc == 1001, (name, rc)
    assert name.encode() in lib.avr_last_error(), lib.avr_last_error()


def test_argument_refusals_without_gpu(lib):
    """Every bad argument is refused (1001, the entry point named in
    avr_last_error) before any device call; the buffers are host memory the
    calls never touch."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    st = None
    nb = ctypes.c_int64(-1)
    fwd, ws, bwd = "avr_group_bias_relu_fwd", "avr_group_bias_relu_workspace", "avr_group_bias_relu_bwd"
    F16 = _lib.DTYPE_F16
    # null pointers (each argument in turn)
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        _refused(lib, fwd, lib.avr_group_bias_relu_fwd(10, 16, 5, 4, args[0], F16, args[1], args[2], args[3], st))
    for k in range(6):
        a = [p] * 6
        a[k] = None
        _refused(lib, bwd, lib.avr_group_bias_relu_bwd(10, 16, 5, 4, a[0], a[1], F16, a[2], a[3], a[4], 1 << 20,
                                                       a[5], st))
    _refused(lib, ws, lib.avr_group_bias_relu_workspace(10, 16, 5, None))
    # W = 12 (not a multiple of 8), W out of range, N % rows_per_group != 0, N <= 0, C <= 0, dtype
    for N, W, rpg, C, dt in ((10, 12, 5, 4, F16), (10, 4, 5, 4, F16), (10, 1032, 5, 4, F16), (10, 16, 4, 4, F16),
                             (0, 16, 5, 4, F16), (10, 16, 5, 0, F16), (10, 16, 5, 4, 7)):
        _refused(lib, fwd, lib.avr_group_bias_relu_fwd(N, W, rpg, C, p, dt, p, p, p, st))
        _refused(lib, bwd, lib.avr_group_bias_relu_bwd(N, W, rpg, C, p, p, dt, p, p, p, 1 << 20, p, st))
    for N, W, rpg in ((10, 12, 5), (10, 16, 4), (0, 16, 5), (10, 2048, 5)):
        _refused(lib, ws, lib.avr_group_bias_relu_workspace(N, W, rpg, ctypes.byref(nb)))
    assert nb.value == -1
    # the workspace size, and a workspace one byte short of it
    assert lib.avr_group_bias_relu_workspace(10, 16, 5, ctypes.byref(nb)) == 0
    assert nb.value == 2 * 1 * 16 * 4  # groups x chunks x W fp32
    assert lib.avr_group_bias_relu_workspace(3 * 4100, 16, 4100, ctypes.byref(nb)) == 0
    assert nb.value >= 3 * 2 * 16 * 4 and nb.value % (3 * 16 * 4) == 0  # more than one chunk per group
    _refused(lib, bwd, lib.avr_group_bias_relu_bwd(3 * 4100, 16, 4100, 4, p, p, F16, p, p, p, nb.value - 1, p, st))
    assert b"workspace" in lib.avr_last_error()


# ---------------------------------------------------------------- tcnn layout
def _pad(n):
    return (n + 15) // 16 * 16


@pytest.mark.parametrize("block", [cc.ADD_DAS, cc.ADD_ALL, cc.CONCAT_ALL, cc.MIXED],
                         ids=["add_das", "add_all", "concat_all", "mixed"])
def test_tcnn_round_trip(block):
    torch.manual_seed(3)
    m = AVRModel(cc.small_model_cfg(block))
    ref = tcnn_compat.to_reference(m)
    own = m.state_dict()
    assert tcnn_compat.is_reference_layout(m, ref) and not tcnn_compat.is_reference_layout(m, own)
    assert not any(k.endswith(".weight") for k in ref)
    for name in ("_model_encoder_sigma", "_model_decoder_sigma", "_model_signal"):
        net = getattr(m, name)
        if isinstance(net, InjectionMLP):
            for i, lin in enumerate(net.hidden_layers):
                k = f"{name}.hidden_layers.{i}.params"
                assert ref[k].shape == (_pad(lin.weight.size(0)) * _pad(lin.weight.size(1)),)
                assert torch.equal(ref[f"{name}.layer_embeddings.{i}"], net.layer_embeddings[i].detach())
            w = net.output_layer.weight
            flat = ref[f"{name}.output_layer.params"]
            assert flat.shape == (_pad(w.size(0)) * _pad(w.size(1)),)
            mat = flat.view(_pad(w.size(0)), _pad(w.size(1)))
            assert torch.equal(mat[:w.size(0), :w.size(1)], w.detach()) and not mat[w.size(0):].any()
            assert f"{name}.params" not in ref
        else:
            n_in = net.layers[0].weight.size(1)
            width = net.layers[0].weight.size(0)
            first = ref[f"{name}.params"][:width * _pad(n_in)].view(width, _pad(n_in))
            assert torch.equal(first[:, :n_in], net.layers[0].weight.detach()) and not first[:, n_in:].any()
    for k in cc.embedding_params(m):
        assert torch.equal(ref[k], own[k])
    torch.manual_seed(4)
    m2 = AVRModel(cc.small_model_cfg(block))
    assert any(not torch.equal(a, b) for a, b in zip(m2.state_dict().values(), own.values()))
    missing, unexpected = tcnn_compat.from_reference(m2, ref)
    assert not missing and not unexpected
    got = m2.state_dict()
    assert got.keys() == own.keys()
    for k in own:
        assert torch.equal(got[k], own[k]), k


def test_tcnn_wrong_size_raises():
    m = AVRModel(cc.small_model_cfg(cc.ADD_DAS))
    ref = tcnn_compat.to_reference(m)
    bad = dict(ref)
    bad["_model_signal.hidden_layers.0.params"] = ref["_model_signal.hidden_layers.0.params"][:-16]
    with pytest.raises(ValueError, match="hidden_layers.0.params"):
        tcnn_compat.from_reference(m, bad)
    bad = dict(ref)
    del bad["_model_encoder_sigma.output_layer.params"]
    with pytest.raises(KeyError):
        tcnn_compat.from_reference(m, bad)


# ---------------------------------------------------------------- ch_idx rules
def test_concat_without_ch_idx_raises():
    m = AVRModel(cc.small_model_cfg(cc.CONCAT_ALL))
    pts = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="ch_idx"):
        m(pts, pts, pts)
    with pytest.raises(ValueError, match="ch_idx"):
        m.forward_fused(pts, pts, pts, ray_layout=(2, 2, 4))
    with pytest.raises(ValueError, match="entries"):
        m(pts, pts, pts, ch_idx=torch.tensor([1, 2, 3]))


def test_kernel_option_and_exports():
    from avr_amd import KernelOptions

    assert KernelOptions().chembed is True and KernelOptions(chembed=False).chembed is False
    for n in ("avr_group_bias_relu_fwd", "avr_group_bias_relu_workspace", "avr_group_bias_relu_bwd"):
        assert n in _lib.EXPORTS
