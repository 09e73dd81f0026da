#!/usr/bin/env python3
"""Makes tests/golden/preview_sequences.json: what tests/test_preview_sequences.py's ``walk`` sees of every configuration
of TemporalPreview on its fixed eleven-frame sequence - digests of the picture, the history, the accumulator's four
records, last_scale and last_motion_code, the phase as it is - and three counts per configuration.  Needs the MI355X.
Run it on the commit whose behaviour is to be kept (it was run on the one before vimg_amd.preview existed); it uses the
preview's public surface only, so the same file runs on either side of such a change.

Every configuration is walked twice, the two in STREAMED a third time on a stream of the caller's; nothing is written
unless all of them agree.

  tests/golden/make_preview_sequences.py [--out FILE]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "preview_sequences.json"))
args = ap.parse_args()

from vimg_amd import hip
import test_preview_sequences as T

hip.init(0)
s = T.panel_scene(res=T.RES)
first = {name: T.walk(s, name) for name in T.CONFIGS}
again = {name: T.walk(s, name) for name in T.CONFIGS}
streamed = {name: T.walk(s, name, streamed=True) for name in T.STREAMED}
differ = [name for name in T.CONFIGS if first[name] != again[name]] + [name + "@stream" for name in T.STREAMED
                                                                       if first[name] != streamed[name]]
for name, run in first.items():
    print(f"{name:40} {run['counts']}", file=sys.stderr)
if differ:
    sys.exit(f"two runs differ, nothing written: {differ}")
lines = ",\n".join(f"{json.dumps(name)}:{json.dumps(run, separators=(',', ':'))}" for name, run in first.items())
with open(args.out, "w") as f:
    f.write(f'{{"res":{T.RES},"items":{json.dumps(list(T.ITEMS))},"streamed":{json.dumps(list(T.STREAMED))},\n'
            f'"configurations":{{\n{lines}\n}}}}\n')
print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes", file=sys.stderr)
