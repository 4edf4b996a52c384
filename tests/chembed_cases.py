"""Shared helpers of the channel-embedding tests (CPU and GPU).

A plain-torch restatement of the reference's injection and concat forward
(model.py:11-61, 183-235), written from its description, with the rounding of
every layer output that tcnn's 16-bit networks apply:

* a tcnn network rounds its input and its weights to the MLP dtype and
  returns its output in that dtype;
* "add": after each bias-free hidden layer `h = float(y) + emb_l[ch]` (the
  fp32 embedding promotes the sum), `x = relu(h)`; the output layer is plain;
  with ch None the add is skipped;
* "concat": the fp32 embedding row of the pose is appended to the network's
  input (to `relu(sigma_feat)` for the decoder);
* `ch_idx` [bs] is expanded over each pose's n rows.

Also the small Real_env model block the tests build, and the six-flag rule
(model.py:71-89) as the expected embedding parameter set.
"""
import json
import math
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = os.path.join(HERE, "golden", "chembed", "configs.json")


def _grid(log2=8):
    return dict(otype="HashGrid", n_levels=20, n_features_per_level=2, log2_hashmap_size=log2, base_resolution=16)


def _net(width, depth=3):
    return dict(otype="CutlassMLP", activation="ReLU", output_activation="None", n_neurons=width,
                n_hidden_layers=depth)


ADD_DAS = dict(is_embed=True, ch_num=8, emb_dim=128, connection_type="add", is_sigma_encoder=True,
               is_sigma_decoder=False, is_signal_network=True)  # the reference's *_add_das block
ADD_ALL = dict(ADD_DAS, is_sigma_decoder=True)
CONCAT_ALL = dict(is_embed=True, ch_num=8, connection_type="concat", is_sigma_encoder=True, is_sigma_decoder=True,
                  is_signal_network=True, emb_dim_sigma_encoder=32, emb_dim_sigma_decoder=32,
                  emb_dim_signal_network=256)
MIXED = dict(CONCAT_ALL, is_sigma_decoder=False)  # concat encoder + signal, plain decoder
NO_MODE = dict(is_embed=True, ch_num=8, emb_dim=128)  # no connection_type: activates nothing


def small_model_cfg(channel_embed=None, widths=(128, 128, 512), depths=(3, 3, 3)):
    """A Real_env `model:` block with small grids: 20 levels, 2^8 entries."""
    cfg = dict(signal_output_dim=254, leaky_relu=0.03,
               pos_encoding_sigma=_grid(), dir_encoding_sig=_grid(), tx_encoding_sig=_grid(),
               sigma_encoder_network=_net(widths[0], depths[0]),
               sigma_decoder_network=_net(widths[1], depths[1]),
               signal_network=_net(widths[2], depths[2]))
    if channel_embed is not None:
        cfg["channel_embed"] = dict(channel_embed)
    return cfg


def load_configs():
    with open(CONFIGS) as f:
        return json.load(f)["configs"]


def expected_embedding_params(block, nets):
    """{parameter name: shape} the six-flag rule gives for a `channel_embed`
    block and the three networks' {n_neurons, n_hidden_layers}."""
    block = block or {}
    on = bool(block.get("is_embed", False))
    conn = block.get("connection_type", None)
    C = block.get("ch_num", 0)
    out = {}
    for flag, net, module, emb, dim in (
            ("is_sigma_encoder", "sigma_encoder_network", "_model_encoder_sigma", "encoder_channel_embedding",
             "emb_dim_sigma_encoder"),
            ("is_sigma_decoder", "sigma_decoder_network", "_model_decoder_sigma", "decoder_channel_embedding",
             "emb_dim_sigma_decoder"),
            ("is_signal_network", "signal_network", "_model_signal", "signal_channel_embedding",
             "emb_dim_signal_network")):
        if not (on and bool(block.get(flag, False))):
            continue
        if conn == "add":
            for i in range(int(nets[net]["n_hidden_layers"])):
                out[f"{module}.layer_embeddings.{i}"] = (C, int(nets[net]["n_neurons"]))
        elif conn == "concat":
            out[emb] = (C, int(block.get(dim, 0)))
    return out


def embedding_params(model):
    return {n: tuple(p.shape) for n, p in model.named_parameters() if "embedding" in n}


# ------------------------------------------------------------ restatement
def _rt(x, dtype):
    return x.to(dtype)


def ref_plain(x, weights, dtype):
    """A bias-free tcnn network: ReLU hidden layers, plain output layer."""
    x = _rt(x, dtype)
    for w in weights[:-1]:
        x = torch.relu(x @ _rt(w, dtype).t())
    return x @ _rt(weights[-1], dtype).t()


def ref_injection(x, hidden, embeddings, output, ch_rows, dtype):
    """LayeredTCNNWithInjection: every layer its own network (16-bit in,
    16-bit out); the embedding add and the ReLU in fp32 between them."""
    for w, e in zip(hidden, embeddings):
        h = _rt(x, dtype) @ _rt(w, dtype).t()
        if ch_rows is not None:
            h = h + e[ch_rows]  # fp32 parameter: the sum is fp32
        x = torch.relu(h)
    return _rt(x, dtype) @ _rt(output, dtype).t()


def _network(model, name, x, table, ch_rows, dtype):
    net = getattr(model, name)
    if hasattr(net, "layer_embeddings"):
        return ref_injection(x, [l.weight for l in net.hidden_layers], list(net.layer_embeddings),
                             net.output_layer.weight, ch_rows, dtype)
    if table is not None and ch_rows is not None:
        x = torch.cat([x, table[ch_rows]], -1)  # promoted to fp32, rounded by the network
    return ref_plain(x, [l.weight for l in net.layers], dtype)


def ref_model(model, pos_enc, dir_enc, tx_enc, ch_idx, n, dtype):
    """AVRModel.forward from the encodings on: (attn [N, 1], signal [N, T])."""
    ch_rows = None if ch_idx is None else ch_idx.long().unsqueeze(1).expand(-1, n).reshape(-1)
    table = lambda k: getattr(model, k, None)  # noqa: E731
    sigma_feat = _network(model, "_model_encoder_sigma", pos_enc, table("encoder_channel_embedding"), ch_rows, dtype)
    attn = _network(model, "_model_decoder_sigma", torch.relu(sigma_feat), table("decoder_channel_embedding"),
                    ch_rows, dtype)
    base = torch.cat([sigma_feat, dir_enc.to(sigma_feat.dtype), tx_enc.to(sigma_feat.dtype)], -1)
    signal = _network(model, "_model_signal", base, table("signal_channel_embedding"), ch_rows, dtype)
    return torch.abs(torch.nn.functional.leaky_relu(attn)), signal


def embedding_init_scale(dim):
    """randn / sqrt(dim): the standard deviation the reference initialises with."""
    return 1.0 / math.sqrt(dim)
