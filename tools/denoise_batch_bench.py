"""Timing of the validation loss with the EDM loss's score-network evaluation batched (``loss_value(..., batched=True)``: ONE
dex_denoise_batch call at B noise levels) against the looped path (a host read of the levels + B dex_denoise_once calls at B = 1).

GeDEXTTS.loss_value (GeDEX-LJ) and DeXTTS.loss_value (DEX-VCTK), synthetic weights, 512 frames (ragged lengths, no cut), B in
{1, 8, 32}, bf16 and fp32 score network; device events after warm-up, median of --iters.

    python tools/denoise_batch_bench.py [--iters 20] [--pairs 3] [--parent DIR] [--out profiles/denoise_batch_bench.json]

--parent DIR: a built checkout of the PARENT commit (a git worktree); its looped loss_value is timed on the same box in alternating
runs with this tree (parent, this, parent, this, ...), one fresh process per run, so that drift hits both alike.  Without it only
this tree is timed (its own batched=False is the same loop).  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(m, B, p) for m in ("gedex_lj", "dex_vctk") for B in (1, 8, 32) for p in ("bf16", "fp32")]
FRAMES, TOKENS = 512, 64


def gpu_ms(fn, iters):
    import numpy as np
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def child(tree, iters, batched):
    """Every configuration on the tree at ``tree``: {"model|B|prec|mode": ms}."""
    sys.path.insert(0, tree)
    os.chdir(tree)
    import numpy as np
    import torch
    from dex_tts_amd import tts
    from tests.test_tts_module import full_state_dict, model_cfg
    out = {}
    models = {}
    for name, B, prec in CONFIGS:
        if name not in models:
            m = (tts.DeXTTS if name.startswith("dex") else tts.GeDEXTTS)(model_cfg(name))
            m.load_state_dict(full_state_dict(m, name))
            models[name] = m.cuda().eval()
        m = models[name]
        m.decoder.precision = prec
        g = torch.Generator().manual_seed(7 + B)
        yl = torch.tensor([FRAMES - (b * 8 * (FRAMES // 2 // 8)) // max(B - 1, 1) for b in range(B)])
        xl = torch.tensor([TOKENS - (b * (TOKENS // 2)) // max(B - 1, 1) for b in range(B)])
        n_vocab = int(model_cfg(name)["n_vocab"])
        args = [torch.randint(1, n_vocab, (B, TOKENS), generator=g).cuda(), xl.cuda(), torch.randn(B, 80, FRAMES, generator=g).cuda(), yl.cuda()]
        kw = dict(rnd_normal=torch.randn(B, 1, 1, generator=g).cuda(), eps=torch.randn(B, 80, FRAMES, generator=g).cuda())
        if name.startswith("dex"):
            Tr = Ts = 96
            rl = torch.tensor([Tr - (b * (Tr // 2)) // max(B - 1, 1) for b in range(B)])
            args += [torch.randn(B, 80, Tr, generator=g).cuda(), rl.cuda(), torch.randn(B, 80, Ts, generator=g).cuda(), rl.cuda(),
                     (5.0 + 0.3 * torch.randn(B, Ts, generator=g)).cuda(), rl.cuda()]
        modes = [("batched", dict(batched=True)), ("looped", {})] if batched else [("looped", {})]
        for mode, extra in modes:
            ms = gpu_ms(lambda: m.loss_value(*args, **kw, **extra), iters)
            out[f"{name}|{B}|{prec}|{mode}"] = ms
    print("CHILD_RESULT " + json.dumps(out))


def run_child(tree, iters, batched):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--iters", str(iters)] + (["--batched"] if batched else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    for line in r.stdout.splitlines():
        if line.startswith("CHILD_RESULT "):
            return json.loads(line[len("CHILD_RESULT "):])
    raise SystemExit(f"child on {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "denoise_batch_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--batched", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.tree, a.iters, a.batched)
    import numpy as np
    import torch
    runs = {"parent": [], "this": []}
    for _ in range(a.pairs):
        if a.parent:
            runs["parent"].append(run_child(os.path.abspath(a.parent), a.iters, False))
        runs["this"].append(run_child(HERE, a.iters, True))
    rows = []
    for name, B, prec in CONFIGS:
        k = f"{name}|{B}|{prec}|"
        bat = [r[k + "batched"] for r in runs["this"]]
        loop = [r[k + "looped"] for r in runs["this"]]
        par = [r[k + "looped"] for r in runs["parent"]]
        row = {"model": name, "B": B, "frames": FRAMES, "precision": prec, "batched_ms": float(np.median(bat)), "batched_runs_ms": bat,
               "looped_ms": float(np.median(loop)), "looped_runs_ms": loop}
        if par:
            row.update(parent_looped_ms=float(np.median(par)), parent_runs_ms=par, parent_spread_ms=float(max(par) - min(par)),
                       batched_over_parent=float(np.median(bat) / np.median(par)))
        rows.append(row)
    out = {"metric": "loss_value_ms", "iters": a.iters, "pairs": a.pairs, "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
