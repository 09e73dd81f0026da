#!/usr/bin/env python3
"""Cost of sparse previews on disney_spheres at 450 x 200 and 1800 x 800, mis, 4 samples a call:
  full        acc.render(4): every pixel takes the increment
  sparse      acc.render(4, mask=lattice) + infill.reconstruct at radius = stride, stride 2 and 4, the phases walked in
              order so every call is one render launch; and Progressive.render_sparse itself, which also builds the mask
              and reads the counts
  fill        the reconstruct call alone (pack + fill), device events around each call; with --other-lib also the same
              call of another build of libvimg_infill.so on the same buffers, the two alternating, and whether the
              two give the same bits (how the LDS-tile form of the fill kernel was measured against the form that
              reads its taps from memory)
  features    the feature render the first call pays (render_features of the four guides at 4 samples)
Host clock around synchronised calls for everything that renders (a render call waits for its launch), medians of
`steps` calls after two warm-up calls, `rounds` rounds alternating the forms.  Prints tables to stderr and one JSON line.

  tools/infill_cost.py [--steps N] [--rounds N] [--other-lib PATH]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=15)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--other-lib", default=None)
args = ap.parse_args()

import numpy as np
import torch
import scenes
from vimg_amd import abi, hip, infill
from _timing import timed, wall

other = abi._bind(C.CDLL(args.other_lib), abi.INFILL_SYMBOLS) if args.other_lib else None


def raw_call(lib, t, count, radius, out, code, work):
    """vimg_infill_reconstruct of `lib` on torch's current stream, on tensors that are already there."""
    frames = abi.InfillFrames(width=out.shape[1], height=out.shape[0], count=count.data_ptr(), **{k: v.data_ptr() for k, v in t.items()})
    p = infill.params(radius=radius)
    rc = lib.vimg_infill_reconstruct(C.byref(frames), C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(code.data_ptr()),
                                     C.c_void_p(work.data_ptr()), work.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.vimg_infill_last_error().decode()


hip.init(0)
res_out = {"steps": args.steps, "rounds": args.rounds, "frames": {}}
name = "disney_spheres.json"
for res in ((450, 200), (1800, 800)):
    w, h = res
    s = scenes.json_scene(name, res=res)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    row = {"features_ms": wall(lambda i: dev.render_features(p, infill.GUIDES), 3)}
    g = dev.render_features(p, infill.GUIDES)
    buf, out = (torch.empty((h, w, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    code = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    work = torch.empty(infill.workspace_bytes(w, h), dtype=torch.uint8, device="cuda")
    full = dev.progressive(p)
    forms = {"full": lambda i: full.render(4, out=buf)}
    accs = [full]
    for stride in (2, 4):
        masks = [infill.lattice_mask(h, w, stride, ph) for ph in range(stride * stride)]
        a_man, a_rs, a_mask = (dev.progressive(p) for _ in range(3))
        accs += [a_man, a_rs, a_mask]
        calls = {"man": 0, "mask": 0}

        def manual(i, a=a_man, masks=masks, stride=stride, calls=calls):
            noisy = a.render(4, out=buf, mask=masks[calls["man"] % len(masks)])
            calls["man"] += 1
            infill.reconstruct(noisy, g["normal"], g["position"], g["depth"], a.counts(), albedo=g["albedo"], radius=stride, out=out,
                               out_code=code, workspace=work)

        def masked(i, a=a_mask, masks=masks, calls=calls):
            a.render(4, out=buf, mask=masks[calls["mask"] % len(masks)])
            calls["mask"] += 1

        forms[f"stride{stride} masked render alone"] = masked
        forms[f"stride{stride} masked render + counts + reconstruct"] = manual
        forms[f"stride{stride} render_sparse"] = lambda i, a=a_rs, stride=stride: a.render_sparse(4, stride=stride, out=out)
    rounds = [{k: wall(fn, args.steps) for k, fn in forms.items()} for _ in range(args.rounds)]
    row["wall_ms_median_of_rounds"] = {k: float(np.median([r[k] for r in rounds])) for k in forms}
    row["wall_ms_rounds"] = rounds
    # the reconstruct call alone, on a frame whose lattice of phase 0 has 4 samples
    row["fill"] = {}
    for stride in (2, 4):
        acc = dev.progressive(p)
        noisy = acc.render(4, mask=infill.lattice_mask(h, w, stride, 0))
        count = acc.counts().to(torch.int32)
        acc.close()
        t = dict(color=noisy, normal=g["normal"], position=g["position"], depth=g["depth"], albedo=g["albedo"])
        for radius in sorted({stride, 2, 4}):
            libs = {"direct": abi.infill_lib()} | ({"other": other} if other else {})
            outs = {k: (torch.empty_like(out), torch.empty_like(code)) for k in libs}
            ms = {k: [] for k in libs}
            for _ in range(args.rounds):               # alternating: other people's work shares the machine
                for k, lib in libs.items():
                    ms[k].append(timed(lambda: raw_call(lib, t, count, radius, *outs[k], work), args.steps))
            torch.cuda.synchronize()
            cell = {k: {"median_ms": float(np.median([m[0] for m in v])), "best_ms": float(min(m[1] for m in v))} for k, v in ms.items()}
            if other:
                cell["same_bits"] = bool(torch.equal(outs["direct"][0].view(torch.int32), outs["other"][0].view(torch.int32))
                                         and torch.equal(outs["direct"][1], outs["other"][1]))
            c = outs["direct"][1]
            cell["codes"] = [float((c == k).float().mean()) for k in range(4)]
            row["fill"][f"stride{stride} radius{radius}"] = cell
    for a in accs:
        a.close()
    dev.close()
    res_out["frames"][f"{w}x{h}"] = row
    print(f"{w} x {h}: feature render {row['features_ms']:.3f} ms", file=sys.stderr)
    for k, v in row["wall_ms_median_of_rounds"].items():
        print(f"  {k:52} {v:8.3f} ms   ({v / row['wall_ms_median_of_rounds']['full']:.3f} of full)", file=sys.stderr)
    for k, cell in row["fill"].items():
        print(f"  reconstruct alone, {k}: " + "   ".join(f"{n} median {cell[n]['median_ms']:.4f} best {cell[n]['best_ms']:.4f} ms"
                                                          for n in ("direct", "other") if n in cell)
              + (f"   same bits: {cell['same_bits']}" if "same_bits" in cell else "")
              + "   codes 0..3: " + " ".join(f"{100 * x:.2f} %" for x in cell["codes"]), file=sys.stderr)
print(json.dumps(res_out))
