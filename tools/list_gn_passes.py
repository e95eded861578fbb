"""List the separate GroupNorm statistics / apply passes left in the 1080p plan (list key, step label)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

dev = torch.device("cuda", 0)
model, _ = bench.build_model(dev)
eng = model._get_engine()
plan = eng.plan(1080, 1920, 1)
for key, S in plan.steps.items():
    for st in S:
        if "gn_apply" in st.label or "gn_stats" in st.label:
            print(key, st.label)
