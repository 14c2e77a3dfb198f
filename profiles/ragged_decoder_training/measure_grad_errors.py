#!/usr/bin/env python3
"""The two measured columns behind the gradient bound of tests/test_gpu_ragged_train.py, per loss case of
tests/ragged_train_ref.py: worst |g - float64 reference| / max |reference| of
  (a) the existing ast_recon_loss_total gradient on the equal-length version of the case (every clip full), and
  (b) the new ast_recon_loss_len_grad gradient on the case itself (ragged), with clip_weights NULL and with the seeded weights.
The test allows (b) <= 4 x max((a), 2^-24).  Both gradients are element-wise, so the figures repeat from run to run.
Usage: python profiles/ragged_decoder_training/measure_grad_errors.py [out.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-style-transfer_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import ragged_train_ref as R  # noqa: E402
import test_gpu_ragged_train as T  # noqa: E402


def main():
    lines = ["case            batch kernel, equal lengths   ragged kernel (1/B)   ragged kernel (weights)   bound = 4 x max(col 1, 2^-24)"]
    for name in T.LOSS_NAMES:
        out, x, o, xd, F, ld, n, parent, bound = T._case(name)
        cols = []
        for weighted in (False, True):
            cw = R.seeded_clip_weights(out.shape[0], seed=len(name)) if weighted else None
            _, ref, _ = R.ragged_loss_ref(out, x[..., :F], n, cw)
            _, _, g = T._raw(o, xd, ld, T._dev_n(n), None if cw is None else torch.from_numpy(cw).to("cuda"))
            cols.append(T._grad_err(g, ref))
        lines.append(f"{name:15s} {parent:12.3e}                  {cols[0]:12.3e}          {cols[1]:12.3e}              {bound:12.3e}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
