"""Settings of every reference config with a `model.channel_embed` block
(build container only; /root/reference is absent on the GPU machine).

Reads every YAML under the reference's `config_files/`, subdirectories
included (most channel configs sit in `real_exp_ch_emb/` and its siblings), and writes
`tests/golden/chembed/configs.json`: for each file with a `channel_embed`
block its path relative to `config_files` (base names repeat between
directories), the block as written, the three networks' `n_neurons` /
`n_hidden_layers`, and the render / train sizes that set the kernel's shape
(`n_azi`, `n_ele`, `n_samples`, `batch_size`).  Settings only, no program
text.  tests/test_chembed_cpu.py builds an `AVRModel` from every entry and
checks its embedding parameters against the reference's six-flag rule
(model.py:71-89).

    python tools/gen_chembed_golden.py
"""
import glob
import json
import os

import yaml

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "chembed", "configs.json")
NETS = ("sigma_encoder_network", "sigma_decoder_network", "signal_network")


def main():
    entries = []
    base = os.path.join(REF, "config_files")
    for path in sorted(glob.glob(os.path.join(base, "**", "*.yml"), recursive=True)):
        with open(path) as f:
            cfg = yaml.safe_load(f)
        model = (cfg or {}).get("model") or {}
        if "channel_embed" not in model:
            continue
        render, train = cfg.get("render") or {}, cfg.get("train") or {}
        entries.append({
            "file": os.path.relpath(path, base),
            "channel_embed": model["channel_embed"],
            "networks": {n: {k: model[n][k] for k in ("n_neurons", "n_hidden_layers")} for n in NETS},
            "signal_output_dim": model.get("signal_output_dim"),
            "n_azi": render.get("n_azi"), "n_ele": render.get("n_ele"), "n_samples": render.get("n_samples"),
            "batch_size": train.get("batch_size"),
        })
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        # one entry per line: 111 entries stay well under 100 KB
        f.write('{"source": "config_files/**/*.yml of the reference (settings only)", "configs": [\n')
        f.write(",\n".join(json.dumps(e, sort_keys=True) for e in entries))
        f.write("\n]}\n")
    print(f"{len(entries)} configs -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
