#!/usr/bin/env python3
"""Golden vectors for the full-set retrieval metrics, produced by running the REFERENCE's own ``get_clip_metrics``
(src/open_clip_train/train.py:383-400) in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_retrieval.py

train.py is loaded by file path; its four package imports (``open_clip.get_input_dtype``, ``open_clip_train.distributed``,
``.zero_shot``, ``.precision``) are stubbed with empty stand-ins at import time -- ``get_clip_metrics`` uses none of them,
and nothing of its arithmetic is replaced.  Writes tests/golden/retrieval_ref.npz: the features, logit_scale and the ten
values the reference returned (inputs and expected outputs only)."""
import sys

sys.dont_write_bytecode = True
import importlib.util
import os
import types

import numpy as np
import torch

REF = os.environ.get("SC_REFERENCE_ROOT", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
N, D, NOISE, LOGIT_SCALE = 300, 16, 0.7, 14.285714149475098       # 1 / 0.07 in fp32


def import_train():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    stub("open_clip", get_input_dtype=lambda *a, **k: None)
    pkg = stub("open_clip_train")
    pkg.__path__ = []
    stub("open_clip_train.distributed", is_master=lambda *a, **k: True)
    stub("open_clip_train.zero_shot", zero_shot_eval=lambda *a, **k: {})
    stub("open_clip_train.precision", get_autocast=lambda *a, **k: None)
    spec = importlib.util.spec_from_file_location("ref_open_clip_train_train", f"{REF}/src/open_clip_train/train.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    train = import_train()
    g = torch.Generator().manual_seed(20)
    fi = torch.nn.functional.normalize(torch.randn(N, D, generator=g, dtype=torch.float64), dim=-1)
    ft = torch.nn.functional.normalize(fi + NOISE * torch.randn(N, D, generator=g, dtype=torch.float64), dim=-1)
    fi, ft = fi.float(), ft.float()
    scale = torch.tensor(LOGIT_SCALE, dtype=torch.float32)
    # the reference's argsort is not stable: an exact tie with a diagonal would leave its answer undefined
    z = scale * fi @ ft.t()
    d = z.diagonal()
    off = ~torch.eye(N, dtype=torch.bool)
    assert not ((z == d[:, None]) & off).any() and not ((z == d[None, :]) & off).any(), "exact tie with a diagonal"
    m = train.get_clip_metrics(fi, ft, scale)
    assert len(m) == 10
    names = sorted(m)
    np.savez(os.path.join(OUT, "retrieval_ref.npz"), image_features=fi.numpy(), text_features=ft.numpy(),
             logit_scale=np.float32(LOGIT_SCALE), names=np.array(names), values=np.array([float(m[k]) for k in names]))
    for k in names:
        print(f"{k:32s} {float(m[k])!r}")


if __name__ == "__main__":
    main()
