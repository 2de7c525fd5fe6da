"""Golden fixture for internvideo_amd.schedules.cosine_scheduler (tests/test_flavours_oracle.py::test_cosine_scheduler_matches_reference).
Needs a checkout of the reference InternVideo repository, named by IV_REFERENCE_ROOT.

Executes the REFERENCE's own `cosine_scheduler` (InternVideo2/single_modality/utils.py:468-485) from its source text on the cases below and
records its schedules (float64, bit-exact) next to the JSON of the cases.

    python tests/golden/make_golden_cosine_scheduler.py      ->  tests/golden/cosine_scheduler.npz     (kwargs, case<i>)
"""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("IV_REFERENCE_ROOT", "")

CASES = [dict(base_value=1.5e-4 * 8, final_value=1e-5 * 8, epochs=5, niter_per_ep=37, warmup_epochs=2, start_warmup_value=1e-6 * 8),
         dict(base_value=0.05, final_value=0.05, epochs=3, niter_per_ep=10),
         dict(base_value=1.0, final_value=0.1, epochs=4, niter_per_ep=25, warmup_epochs=1, warmup_steps=7)]


def load_reference():
    assert os.path.isdir(REF), "set IV_REFERENCE_ROOT to a checkout of the reference repository"
    src = open(os.path.join(REF, "InternVideo2", "single_modality", "utils.py")).read()
    body = src[src.index("def cosine_scheduler("):src.index("def save_model(")]
    ns = {"np": np, "math": math, "print": lambda *a, **k: None}
    exec(compile(body, "utils_extract", "exec"), ns)
    return ns["cosine_scheduler"]


def main():
    fn = load_reference()
    d = {"kwargs": np.array(json.dumps(CASES))}
    for i, kw in enumerate(CASES):
        d[f"case{i}"] = np.asarray(fn(**kw), dtype=np.float64)
    path = os.path.join(HERE, "cosine_scheduler.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}: {', '.join(f'{k} {v.shape}' for k, v in d.items())}")


if __name__ == "__main__":
    main()
