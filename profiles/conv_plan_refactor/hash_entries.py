"""SHA-256 of what every row of tests/igemm_cases.CASES stores, launched through ops._igemm on the row's seeded inputs under the
row's environment.  MI355X; run once per library in a process of its own:

    AST_HIP_LIB=<parent or new libast_hip.so> python profiles/conv_plan_refactor/hash_entries.py > hashes_<build>.txt

Per row: a plain launch (bias), a launch that accumulates into the seeded previous destination with ReLU, and the deterministic
form.  A split-K row adds its slices with f32 atomics in the default mode, in an order that changes from launch to launch, so
its default-mode lines hash only the pixels off the launch's grid (which no launch may touch); its deterministic line hashes
everything.  `diff` of the two builds' outputs must be empty."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "audio-style-transfer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from ast_amd import _lib, config, ops  # noqa: E402
import igemm_cases as IC  # noqa: E402

DEV = "cuda:0"


def digest(t, keep=None):
    t = t.detach().float().cpu()
    if keep is not None:
        t = t[:, keep, :]
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def main():
    for case in IC.CASES:
        g = case.gather()
        v = {k: t.to(DEV) for k, t in IC.make_inputs(case).items()}
        off_grid = ~IC.grid_mask(g) if case.ws > 0 else None
        with IC.case_env(case):
            assert IC.plan_of(g, case.dtype) == (case.plan, case.ws), case.name
            out = []
            for det in (False, True):
                config.deterministic = det
                ops._ws_cache.clear()
                keep = None if det else off_grid
                y = v["old"].clone()
                ops._igemm(v["src"], v["wgt"], v["bias"], y, g)
                out.append(digest(y, keep))
                if not det:
                    y = v["old"].clone()
                    ops._igemm(v["src"], v["wgt"], None, y, g, flags=_lib.IGEMM_ACCUMULATE | _lib.IGEMM_RELU)
                    out.append(digest(y, keep))
            config.deterministic = False
        torch.cuda.synchronize()
        print(f"{case.name} plain {out[0]} acc_relu {out[1]} det {out[2]}", flush=True)


if __name__ == "__main__":
    main()
