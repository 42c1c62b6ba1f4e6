"""Shared cases of the window-contract mask / patch tests (tests/test_window_mask_cpu.py, _gpu.py): the
batches, the oracle's logits and gradients for them (computed once per process) and the comparison.

The oracle takes `eeg_mask` as the token mask and knows no patches, so for it the window is prepared
with plain torch: masked steps zeroed and, for P > 1, the window pre-patched to [B, C*P, L] (row c*P + p
of token j = channel c, step j*P + p), which its per-step eeg_encoder then reads as the patch GEMM."""
from __future__ import annotations

import functools

import torch

from goldens import SEED, det_params
from oracle import fusion_oracle as O
from oracle.detweights import det_tensor

C, A = 64, 32
# name -> window length T, patch P, valid steps per row (a prefix), hole (row, first, last+1) or None
CASES = {
    "prefix": dict(T=200, P=1, lens=(200, 137, 1), hole=None),
    "hole": dict(T=200, P=1, lens=(200, 137, 1), hole=(0, 50, 90)),
    # 301 = 75 patches + 1 step and 6 = 1 patch + 2 steps: the last token of rows 1, 2 is partly valid
    "patch4": dict(T=512, P=4, lens=(512, 301, 6), hole=None),
    "pg4": dict(T=200, P=1, lens=(200, 137, 1, 64), hole=None),
    "t128": dict(T=128, P=1, lens=(128, 128), hole=None),          # every step valid: run without a mask
    "t256": dict(T=256, P=1, lens=(256, 256), hole=None),
    "t256m": dict(T=256, P=1, lens=(256, 100, 31), hole=None),
}


def step_mask(T, lens, hole=None):
    m = torch.zeros(len(lens), T, dtype=torch.int64)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    if hole is not None:
        m[hole[0], hole[1]:hole[2]] = 0
    return m


@functools.lru_cache(maxsize=None)
def batch(case: str):
    """host tensors of a case: eeg [B, C, T], act [B, A], labels, step mask, noise / gumbels (PriGumbel)"""
    c = CASES[case]
    B = len(c["lens"])
    g = torch.Generator().manual_seed(1234 + sorted(CASES).index(case))
    eeg = torch.randn(B, C, c["T"], generator=g)
    act = torch.randn(B, A, generator=g) * 0.5
    labels = torch.randint(0, 2, (B,), generator=g)
    noise = O.laplace_from_uniform(torch.rand(B, O.FUSED, generator=g) * 2 - 1)
    gumbels = -torch.log(-torch.log(torch.rand(2, B, O.FUSED, generator=g).clamp(1e-6, 1 - 1e-6)))
    return dict(eeg=eeg, act=act, labels=labels, mask=step_mask(c["T"], c["lens"], c["hole"]), noise=noise,
                gumbels=gumbels, P=c["P"])


def params(variant: str, patch: int, requires_grad: bool):
    p = det_params("W", variant, requires_grad=False)
    if patch > 1:
        p["eeg_encoder.weight"] = torch.from_numpy(det_tensor(SEED, "eeg_encoder.weight", (O.HID, C * patch)).copy())
    for t in p.values():
        t.requires_grad_(requires_grad)
    return p


def oracle_inputs(eeg, mask, patch):
    """the oracle's batch entries for a masked / patched window: (eeg', token mask)"""
    B, Cc, T = eeg.shape
    L = T // patch
    eeg = torch.where(mask[:, None, :] != 0, eeg, torch.zeros(()))
    eeg = eeg.view(B, Cc, L, patch).permute(0, 1, 3, 2).reshape(B, Cc * patch, L)
    return eeg, (mask.view(B, L, patch) != 0).any(-1).long()


@functools.lru_cache(maxsize=None)
def oracle(variant: str, case: str, hard: bool = False):
    """-> (logits [B, 2], {name: gradient}) of the oracle on the case, mean cross-entropy loss"""
    bt = batch(case)
    p = params(variant, bt["P"], True)
    eeg, tmask = oracle_inputs(bt["eeg"], bt["mask"], bt["P"])
    pc = O.PathConfig(contract="W", variant=variant, eps=1.0, hard=hard)
    logits = O.forward(p, dict(eeg=eeg, act=bt["act"], eeg_mask=tmask), pc, noise=bt["noise"], gumbels=bt["gumbels"])
    assert bool(torch.isfinite(logits).all())
    torch.nn.functional.cross_entropy(logits, bt["labels"]).backward()
    return logits.detach(), {n: t.grad.detach() for n, t in p.items() if t.grad is not None}


def build(variant: str, patch: int = 1, **kw):
    """the module under test with the deterministic weights (dropout 0, fp32, host memory)"""
    from eegfusion.modules import ConcatModel, PriGumbelModel
    torch.manual_seed(0)
    if variant == "prigumbel":
        m = PriGumbelModel(1.0, contract="W", dropout=0.0, eeg_patch=patch, **kw)
    else:
        m = ConcatModel(contract="W", dropout=0.0, eeg_patch=patch, **kw)
    m.load_state_dict(params(variant, patch, False), strict=False)
    return m.train()


def run(m, case: str, hard: bool = False, dev: str = "cpu", mask="case"):
    """forward_window + mean CE backward of module m on the case -> (logits, {name: grad}) on the host"""
    bt = batch(case)
    m.engine.injected = dict(noise=bt["noise"].to(dev), gumbels=bt["gumbels"].to(dev).contiguous())
    msk = bt["mask"].to(dev) if isinstance(mask, str) else mask
    logits = m.forward_window(bt["eeg"].to(dev), bt["act"].to(dev), hard, eeg_mask=msk)
    torch.nn.functional.cross_entropy(logits, bt["labels"].to(dev)).backward()
    if dev != "cpu":
        torch.cuda.synchronize()
    return logits.detach().double().cpu(), {n: q.grad.detach().double().cpu() for n, q in m.named_parameters()
                                            if q.grad is not None}


def rel(a, b) -> float:
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))


def check(logits, grads, ref_logits, ref_grads, ltol: float, gtol: float):
    """logits within ltol and every gradient the reference has within gtol, both relative to the
    reference tensor's largest magnitude; structurally zero gradients (softmax shift invariance: the
    attention key biases, the decoder's single-key self-attention q / k) hold rounding residue only"""
    e = rel(logits, ref_logits)
    print(f"logits rel err {e:.3e}")
    assert e < ltol, e
    bad, worst = [], 0.0
    for n, r in ref_grads.items():
        g = grads.get(n)
        if float(r.abs().max()) < 1e-7:
            if g is not None and float(g.abs().max()) > 1e-6:
                bad.append((n, "expected ~0", float(g.abs().max())))
            continue
        if g is None:
            bad.append((n, "missing"))
            continue
        e = rel(g.reshape(r.shape), r)
        worst = max(worst, e)
        if e >= gtol:
            bad.append((n, e))
    print(f"worst gradient rel err {worst:.3e}")
    assert not bad, bad[:10]
