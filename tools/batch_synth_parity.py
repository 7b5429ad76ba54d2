"""The yardstick for the batched text -> mel path's mel bar (tests/test_batch_synth_gpu.py): how far does the
EXISTING batching move a mel?  Run on the commit that has no `mel_ragged` yet; it uses nothing newer than `eval_front` / `eval_back`,
the two halves `GraphedSynthesizer.mel` replays.

Four texts of equal length L run as one (4, L) block and each alone as (1, L).  Rows whose frame count T_u is below the block's T
carry the reference's PostNet end effect in the block (mel_linear's bias in their padded frames, Layers.py:133-143): a semantic
difference, not rounding.  So the postnet mel is compared on frames t < T_u - 10 only (five k = 5 layers reach 10 frames) and the
pre-PostNet mel on all valid frames.  The largest rel-RMS over the rows is the yardstick; the new path is held to twice that on
ALL valid frames of both mels (torch.equal if it is exactly 0).

usage: python tools/batch_synth_parity.py [--out profiles/batch_synth_parity.json] [--commit HASH]
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).pow(2).mean() / b.pow(2).mean().clamp_min(1e-30)).sqrt())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_synth_parity.json"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    from tts_king_amd.config import default_config
    from tts_king_amd.fastspeech2 import FastSpeech2
    cfg = default_config()
    dev = "cuda:0"
    m = FastSpeech2(cfg.preprocess_config, cfg.model_config, 66, device=dev)
    with torch.no_grad():
        m.get("variance_adaptor.duration_predictor.linear_layer.bias").fill_(1.3)
    m.eval()
    speakers = torch.tensor([5, 9, 2, 30], device=dev)
    rows = []
    worst = 0.0
    with torch.no_grad():
        for L, seed in ((40, 5),):
            g = torch.Generator().manual_seed(seed)
            texts = torch.randint(1, 207, (4, L), generator=g).to(dev)
            lens = torch.full((4,), L, dtype=torch.int64, device=dev)
            x3, dur, total, _ = m.eval_front(speakers, texts, lens, L)
            T = max(int(total.max().item()), 1)
            mel_b, post_b, ml_b, _ = m.eval_back(x3, dur, L, T)
            for u in range(4):
                x3s, durs, tots, _ = m.eval_front(speakers[u:u + 1], texts[u:u + 1], lens[:1], L)
                Tu = max(int(tots.max().item()), 1)
                mel_s, post_s, _, _ = m.eval_back(x3s, durs, L, Tu)
                same_T = Tu == int(ml_b[u]) and torch.equal(dur.view(4, L)[u], durs.view(-1))      # else the rows share no frame positions
                r_mel = rel_rms(mel_b[u, :Tu], mel_s[0]) if same_T else None
                n = Tu if Tu == T else Tu - 10
                r_post = rel_rms(post_b[u, :n], post_s[0, :n]) if same_T and n > 0 else None
                rows.append({"L": L, "row": u, "T_row": Tu, "T_block": T, "durations_equal": bool(same_T),
                             "mel_rel_rms": r_mel, "postnet_rel_rms_inner": r_post,
                             "mel_bit_equal": bool(same_T and torch.equal(mel_b[u, :Tu], mel_s[0]))})
                print(rows[-1])
                worst = max(worst, r_mel or 0.0, r_post or 0.0)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
        except Exception:
            commit = "unknown"
    out = {"what": "largest rel-RMS between a mel from a (4, L) block and the same text as (1, L), GraphedSynthesizer.mel's two halves, "
                   "pre-PostNet mel on all valid frames and postnet mel on frames t < T_u - 10",
           "commit": commit, "yardstick_rel_rms": worst, "bar_for_the_batched_path": 2 * worst, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("yardstick rel-RMS %.3e -> %s" % (worst, a.out))


if __name__ == "__main__":
    main()
