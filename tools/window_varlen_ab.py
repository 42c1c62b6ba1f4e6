"""Packed against padded on a masked window batch, and the patch-token kernel against eegf_window_tokens.

Step: the bench workload's shape (bf16 PriGumbel step, B = 256, C = 64, T = 256, dropout 0.1) with seeded
prefix lengths uniform in [lo, hi] (default [64, 256], about 62 % valid tokens), run three ways in one
process, interleaved in rounds so that clock drift cannot favour one: the packed route (cfg.varlen =
True: BERT over the valid tokens only), the padded route (cfg.varlen = False: B * L rows + key bias, the
dense attention kernels) and the unmasked batch (today's route) for scale.  Each round warms a route up
with 2 steps, then times `--steps` steps between device events.  Median ms / step per route.

Kernel: eegf_window_patch_tokens (no mask / step mask / packed rows) and eegf_window_tokens at the same
shape, `--iters` launches between device events after a warm-up; GB/s over the algorithmic bytes (the
fp32 window read once, the bf16 rows written once; the int64 step mask where one is read).

Usage: python tools/window_varlen_ab.py [--rounds 5] [--steps 8] [--out profiles/window_varlen_ab.json]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "eeg-multimodal_amd"), str(ROOT)]
import torch  # noqa: E402


def _timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def _median(x):
    x = sorted(x)
    return x[len(x) // 2]


def step_ab(args, dev):
    from eegfusion.modules import PriGumbelModel
    from eegfusion.trainer import PriGumbelTrainer
    B, C, T = args.batch, 64, args.T
    torch.manual_seed(980616)
    m = PriGumbelModel(1.0, contract="W", dropout=0.1).to(dev).set_compute_dtype(torch.bfloat16)
    tr = PriGumbelTrainer(m.engine, lr=1e-6)
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(args.lo, args.hi + 1, (B,), generator=g)
    mask = (torch.arange(T)[None, :] < lens[:, None]).to(torch.int64).to(dev)
    gd = torch.Generator(device=dev).manual_seed(7)
    eeg = torch.randn(B, C, T, generator=gd, device=dev)
    act = torch.randn(B, 32, generator=gd, device=dev) * 0.5
    labels = (torch.rand(B, generator=gd, device=dev) < 0.66).long()
    routes = {"packed": (True, {"eeg": eeg, "act": act, "eeg_mask": mask}),
              "padded": (False, {"eeg": eeg, "act": act, "eeg_mask": mask}),
              "unmasked": (True, {"eeg": eeg, "act": act})}
    res = {k: [] for k in routes}
    for _ in range(args.rounds):
        for name, (varlen, batch) in routes.items():
            m.engine.cfg.varlen = varlen
            for _ in range(2):
                tr.step(batch, labels)
            torch.cuda.synchronize()
            # a new mask tensor every step, as a data loader delivers it: the plan (one small device-to-host
            # copy) is made once per step and is part of the step time
            res[name].append(_timed(lambda: tr.step({k: v.clone() if k == "eeg_mask" else v for k, v in batch.items()},
                                                    labels), args.steps))
    share = float(lens.sum()) / (B * T)
    rows = (int(lens.sum()) + 255) // 256 * 256
    out = {"B": B, "C": C, "T": T, "lens": [args.lo, args.hi], "valid_token_share": round(share, 4),
           "packed_rows": rows, "padded_rows": B * T, "row_share": round(rows / (B * T), 4)}
    for name in routes:
        out[name + "_ms"] = round(_median(res[name]), 3)
        out[name + "_all_ms"] = [round(t, 3) for t in res[name]]
    out["packed_over_padded"] = round(out["packed_ms"] / out["padded_ms"], 4)
    return out, mask, lens


def kernel_ab(args, dev, mask, lens):
    from eegfusion import _lib
    B, C, T = args.batch, 64, args.T
    s = torch.cuda.current_stream().cuda_stream
    eeg = torch.randn(B, C, T, device=dev)
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = lens.cumsum(0).to(torch.int32)
    n = int(cu[-1])
    R = (n + 255) // 256 * 256
    cu = cu.to(dev)
    tok = torch.empty(B * T, C, dtype=torch.bfloat16, device=dev)
    e, o, mp, cp = eeg.data_ptr(), tok.data_ptr(), mask.data_ptr(), cu.data_ptr()
    full = B * C * T * 4 + B * T * C * 2
    runs = {
        "window_tokens": (lambda: _lib.call("eegf_window_tokens", _lib.BF16, B, C, T, e, o, s), full),
        "patch_tokens": (lambda: _lib.call("eegf_window_patch_tokens", _lib.BF16, B, C, T, 1, None, None, B * T, B * T,
                                           e, o, s), full),
        "patch_tokens_masked": (lambda: _lib.call("eegf_window_patch_tokens", _lib.BF16, B, C, T, 1, mp, None, B * T,
                                                  B * T, e, o, s), n * C * 4 + B * T * C * 2 + B * T * 8),
        "patch_tokens_packed": (lambda: _lib.call("eegf_window_patch_tokens", _lib.BF16, B, C, T, 1, mp, cp, n, R, e, o,
                                                  s), n * C * 4 + R * C * 2 + B * T * 8),
    }
    out = {}
    for _ in range(args.rounds):
        for name, (fn, _b) in runs.items():
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            out.setdefault(name, []).append(_timed(fn, args.iters))
    return {name: {"us": round(_median(out[name]) * 1e3, 2), "bytes": runs[name][1],
                   "GBps": round(runs[name][1] / (_median(out[name]) * 1e-3) / 1e9, 1)} for name in runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--lo", type=int, default=64)
    ap.add_argument("--hi", type=int, default=256)
    ap.add_argument("--out", default="profiles/window_varlen_ab.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_varlen_ab: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda")
    step, mask, lens = step_ab(args, dev)
    res = {"step": step, "kernel": kernel_ab(args, dev, mask, lens)}
    print(json.dumps(res, indent=1), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
