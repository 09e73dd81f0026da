#!/usr/bin/env python3
"""Makes tests/golden/cu_launch_plans.json: for every case of tests/test_launch_plan.py's CASES the inputs and the complete
plan the launch planner makes of them (the test's own program around v-img_amd/csrc/launch_plan.hip, compiled for the
host alone).  Needs hipcc and no GPU.

The file in the repository was first written on the commit before the planner existed: there the same cases went
through launch_policy.hip's make_launch, compiled for the host alone with stub kernel getters and a device scene filled
from the same fields (the occupancy queries fail without a device and fall back to one workgroup per compute unit,
which is the `lane_per_cu` of every case).  This script must reproduce that file byte for byte; run it again only
to add cases, and then on a commit whose plans are to be kept.

  tests/golden/make_cu_launch_plans.py [--out FILE]"""
import argparse
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "cu_launch_plans.json"))
args = ap.parse_args()

import test_launch_plan as T

with tempfile.TemporaryDirectory() as d:
    exe = T.build_program(d)
    first = T.run_plans(exe, list(T.CASES.values()))
    again = T.run_plans(exe, list(T.CASES.values()))
if first != again:
    sys.exit("two runs differ, nothing written")
with open(args.out, "w") as f:
    f.write(T.record_text(first))
print(f"wrote {args.out}: {len(first)} cases, {os.path.getsize(args.out)} bytes", file=sys.stderr)
