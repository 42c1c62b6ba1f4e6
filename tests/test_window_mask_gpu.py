"""Window contract at any length, with a step mask and a patch tokenizer, on the GPU.

  * the new front-end kernels (eegf_window_patch_tokens, eegf_window_token_mask, eegf_packed_pos_rows)
    against torch indexing, exact equality (the cast is the only rounding);
  * the engine against the oracle, fp32, logits and every parameter gradient within 1e-4 of the tensor's
    largest magnitude (the bound of tests/test_model_gpu.py), on each route: packed rows (prefix masks),
    padded + key bias (a hole), the patch tokenizer, the varlen kernels on the padded layout (T = 128);
  * packed == padded (cfg.varlen on / off) at the bounds of tests/test_varlen_gpu.py;
  * no mask == all-ones mask at T = 256, bit for bit, with dropout on;
  * the trainer makes the mask plan once per step; a DP-SGD step runs on the padded route.
The cases and the oracle's values are shared with tests/test_window_mask_cpu.py (tests/window_cases.py)."""
import pytest
import torch

import window_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _s():
    return torch.cuda.current_stream().cuda_stream


def _counts(fn):
    from eegfusion import _lib
    torch.cuda.synchronize()
    _lib.lib().eegf_launch_log_reset()
    out = fn()
    torch.cuda.synchronize()
    return out, _lib.launch_counts()


def _n(counts, kernel):
    return sum(v for k, v in counts.items() if kernel in k)


# ------------------------------------------------------------------------------------ kernels
SHAPES = [(3, 64, 200, 1), (2, 30, 96, 1), (2, 64, 512, 4), (2, 16, 64, 8), (1, 128, 64, 8)]


def _steps(B, T, P):
    """valid steps per row: a prefix that ends inside a patch (for P > 1), the whole row, a single step"""
    n = [T * 3 // 5 + 1, T, 1][:B]
    if P > 1 and n[0] % P == 0:
        n[0] += 1
    return n


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B, C, T, P", SHAPES)
def test_window_patch_tokens_kernel(B, C, T, P, dt):
    from eegfusion import _lib as lib
    code = lib.F32 if dt == torch.float32 else lib.BF16
    g = torch.Generator().manual_seed(B * 1000 + C + T + P)
    eeg = torch.randn(B, C, T, generator=g).to(DEV)
    L, W = T // P, C * P
    steps = _steps(B, T, P)
    mask = wc.step_mask(T, steps).to(DEV)
    tlens = [(n + P - 1) // P for n in steps]
    # garbage in the masked steps must not reach a token
    dirty = torch.where(mask[:, None, :] != 0, eeg, torch.full((), float("nan"), device=DEV))
    ref = torch.where(mask[:, None, :] != 0, eeg, torch.zeros((), device=DEV))
    ref = ref.view(B, C, L, P).permute(0, 2, 1, 3).reshape(B, L, W).to(dt)
    # token mask
    tm = torch.full((B, L), 7, dtype=torch.int64, device=DEV)
    lib.call("eegf_window_token_mask", B, T, P, mask.data_ptr(), tm.data_ptr(), _s())
    assert torch.equal(tm, (mask.view(B, L, P) != 0).any(-1).long())
    assert tm.sum(1).tolist() == tlens
    # padded layout, mask applied (a hole through a patch in row 0 as well)
    hole = mask.clone()
    hole[0, 3:3 + P + 1] = 0
    refh = torch.where(hole[:, None, :] != 0, eeg, torch.zeros((), device=DEV))
    refh = refh.view(B, C, L, P).permute(0, 2, 1, 3).reshape(B * L, W).to(dt)
    R = (B * L + 255) // 256 * 256 + 256
    out = torch.full((R, W), 3.0, device=DEV).to(dt)
    lib.call("eegf_window_patch_tokens", code, B, C, T, P, hole.data_ptr(), None, B * L, R, dirty.data_ptr(),
             out.data_ptr(), _s())
    assert torch.equal(out[:B * L], refh)
    assert torch.count_nonzero(out[B * L:].float()) == 0
    # padded layout, no mask
    out = torch.full((B * L, W), 3.0, device=DEV).to(dt)
    lib.call("eegf_window_patch_tokens", code, B, C, T, P, None, None, B * L, B * L, eeg.data_ptr(), out.data_ptr(),
             _s())
    assert torch.equal(out, eeg.view(B, C, L, P).permute(0, 2, 1, 3).reshape(B * L, W).to(dt))
    # packed layout
    cu = torch.tensor([0] + torch.tensor(tlens).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    n = int(cu[-1])
    R = (n + 255) // 256 * 256
    out = torch.full((R, W), 3.0, device=DEV).to(dt)
    lib.call("eegf_window_patch_tokens", code, B, C, T, P, mask.data_ptr(), cu.data_ptr(), n, R, dirty.data_ptr(),
             out.data_ptr(), _s())
    torch.cuda.synchronize()
    for b, ln in enumerate(tlens):
        assert torch.equal(out[int(cu[b]):int(cu[b]) + ln], ref[b, :ln]), b
    assert torch.count_nonzero(out[n:].float()) == 0
    # packed position rows
    pos = torch.randn(512, 768, generator=g).to(DEV)
    pr = torch.full((R, 768), 3.0, device=DEV)
    lib.call("eegf_packed_pos_rows", B, L, 768, cu.data_ptr(), n, R, pos.data_ptr(), pr.data_ptr(), _s())
    for b, ln in enumerate(tlens):
        assert torch.equal(pr[int(cu[b]):int(cu[b]) + ln], pos[:ln])
    assert torch.count_nonzero(pr[n:]) == 0


def test_front_end_argument_errors():
    from eegfusion import _lib
    lib = _lib.lib()
    x = torch.zeros(2 * 64 * 64, device=DEV)
    m = torch.ones(2 * 64, dtype=torch.int64, device=DEV)
    cu = torch.tensor([0, 64, 128], dtype=torch.int32, device=DEV)
    y = torch.zeros_like(x)
    e, o, mp, cp = x.data_ptr(), y.data_ptr(), m.data_ptr(), cu.data_ptr()

    def tok(dtype=0, B=2, C=64, T=64, P=1, mask=mp, cu_=None, packed=128, total=128, eeg=e, out=o):
        return lib.eegf_window_patch_tokens(dtype, B, C, T, P, mask, cu_, packed, total, eeg, out, _s())
    assert tok() == 0
    for bad in (dict(dtype=2), dict(B=0), dict(C=129), dict(C=0), dict(P=3), dict(P=16), dict(T=63, P=2),
                dict(eeg=None), dict(out=None), dict(packed=129, total=129), dict(packed=100), dict(total=127), dict(packed=0, cu_=cp)):
        assert tok(**bad) == _lib.ERR_ARG, bad
    assert lib.eegf_window_token_mask(2, 64, 2, mp, o, _s()) == 0
    assert lib.eegf_window_token_mask(2, 64, 3, mp, o, _s()) == _lib.ERR_ARG
    assert lib.eegf_window_token_mask(2, 63, 2, mp, o, _s()) == _lib.ERR_ARG
    assert lib.eegf_window_token_mask(2, 64, 2, None, o, _s()) == _lib.ERR_ARG
    assert lib.eegf_packed_pos_rows(2, 64, 770, cp, 128, 128, e, o, _s()) == _lib.ERR_ARG
    assert lib.eegf_packed_pos_rows(2, 64, 768, None, 128, 128, e, o, _s()) == _lib.ERR_ARG
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- engine vs oracle
def _dev_model(variant, patch=1, dtype=torch.float32, dropout=None):
    m = wc.build(variant, patch).cuda().train()
    if dtype != torch.float32:
        m.set_compute_dtype(dtype)
    if dropout is not None:
        c = m.engine.cfg
        c.hidden_dropout = c.attn_dropout = c.dec_dropout = dropout
    return m


@pytest.mark.parametrize("variant", ["concat", "prigumbel"])
@pytest.mark.parametrize("case", ["prefix", "hole", "patch4"])
def test_masked_window_vs_oracle_fp32(variant, case):
    m = _dev_model(variant, wc.CASES[case]["P"])
    (logits, grads), counts = _counts(lambda: wc.run(m, case, dev=DEV))
    wc.check(logits, grads, *wc.oracle(variant, case), 1e-4, 1e-4)
    # the routes: prefix masks run BERT over the packed rows, a hole keeps the padded layout
    assert _n(counts, "window_patch_tokens_kernel") == 1 and _n(counts, "window_tokens_kernel") == 0
    assert _n(counts, "seq_lengths_kernel") == 1
    assert _n(counts, "packed_pos_rows_kernel") == (0 if case == "hole" else 1)
    assert _n(counts, "window_token_mask_kernel") == (1 if case == "patch4" else 0)


def test_packed_rows_skip_the_padding():
    """the packed route's BERT rows are the valid tokens rounded up to 256, not B * L"""
    m = _dev_model("concat")
    bt = wc.batch("prefix")
    batch = {"eeg": bt["eeg"].to(DEV), "act": bt["act"].to(DEV), "eeg_mask": bt["mask"].to(DEV)}
    with torch.no_grad():
        _, sv = m.engine.forward(batch, True, False, save=False)
        assert sv.R == 512 and sv.vl is not None and not sv.vl.get("uniform") and sv.vl["T"] == 338
        m.engine.cfg.varlen = False
        _, sv = m.engine.forward(batch, True, False, save=False)
        assert sv.R == 600 and sv.vl.get("uniform")
    torch.cuda.synchronize()


def test_t128_without_mask_forward_and_backward():
    m = _dev_model("concat")
    logits, grads = wc.run(m, "t128", dev=DEV, mask=None)
    wc.check(logits, grads, *wc.oracle("concat", "t128"), 1e-4, 1e-4)


@pytest.mark.parametrize("hard", [False, True])
def test_prigumbel_t200_vs_oracle_fp32(hard):
    m = _dev_model("prigumbel")
    logits, grads = wc.run(m, "pg4", hard=hard, dev=DEV)
    wc.check(logits, grads, *wc.oracle("prigumbel", "pg4", hard), 1e-4, 1e-4)


# ----------------------------------------------------------------------------- packed == padded
def _run_varlen(varlen, dtype):
    m = _dev_model("concat", dtype=dtype)
    m.engine.cfg.varlen = varlen
    return wc.run(m, "pg4", dev=DEV)


def test_packed_equals_padded_fp32():
    lp, gp = _run_varlen(False, torch.float32)
    lv, gv = _run_varlen(True, torch.float32)
    assert wc.rel(lv, lp) < 1e-5
    assert set(gp) == set(gv)
    for n in gp:
        if n.endswith("attention.self.key.bias"):
            scale = gp[n.replace("key.bias", "query.bias")].abs().max().item()
            assert gv[n].abs().max().item() <= 1e-4 * scale and gp[n].abs().max().item() <= 1e-4 * scale, n
            continue
        den = max(gp[n].abs().max().item(), 1e-30)
        assert (gv[n] - gp[n]).abs().max().item() / den < 1e-4, n


def test_packed_equals_padded_bf16():
    lp, gp = _run_varlen(False, torch.bfloat16)
    lv, gv = _run_varlen(True, torch.bfloat16)
    assert wc.rel(lv, lp) < 2e-2
    for n in ("bert.encoder.layer.0.attention.self.query.weight", "bert.encoder.layer.11.output.dense.weight",
              "eeg_encoder.weight", "eeg_encoder.bias", "bert.embeddings.position_embeddings.weight",
              "fc_layers.0.weight"):
        a, b = gv[n].flatten(), gp[n].flatten()
        cos = (a @ b / (a.norm() * b.norm())).item()
        assert cos >= 0.999, (n, cos)


# ----------------------------------------------------------------------------- no behaviour change
def test_all_ones_mask_is_bitwise_no_mask():
    """T = 256, P = 1, dropout 0.1: eeg_mask=None and an all-ones mask launch the same kernels and give the
    same bits (engine.rng_counter reset between the runs so both draw the same dropout masks)"""
    m = _dev_model("prigumbel", dropout=0.1)
    r0 = m.engine.rng_counter
    runs = []
    for mask in (None, torch.ones(2, 256, dtype=torch.bool, device=DEV)):
        for q in m.parameters():
            q.grad = None
        m.engine.rng_counter = r0
        (logits, grads), counts = _counts(lambda: wc.run(m, "t256", hard=True, dev=DEV, mask=mask))
        counts = {k: v for k, v in counts.items() if "seq_lengths_kernel" not in k}
        runs.append((logits, grads, counts))
    (l0, g0, c0), (l1, g1, c1) = runs
    assert c0 == c1 and _n(c0, "window_tokens_kernel") == 1 and _n(c0, "window_patch_tokens_kernel") == 0
    assert torch.equal(l0, l1) and set(g0) == set(g1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ----------------------------------------------------------------------------- trainer, DP-SGD
def test_trainer_makes_the_plan_once_per_step():
    from eegfusion.trainer import PriGumbelTrainer
    m = _dev_model("prigumbel", dropout=0.1)
    tr = PriGumbelTrainer(m.engine, lr=1e-4)
    bt = wc.batch("pg4")
    before = m.eeg_encoder.weight.detach().clone()

    def two_steps():
        for _ in range(2):         # a new mask tensor per step, shared by the step's two forwards
            batch = {"eeg": bt["eeg"].to(DEV), "act": bt["act"].to(DEV), "eeg_mask": bt["mask"].to(DEV)}
            loss, _ = tr.step(batch, bt["labels"].to(DEV))
        return loss.clone()
    loss, counts = _counts(two_steps)
    assert _n(counts, "seq_lengths_kernel") == 2
    assert _n(counts, "window_patch_tokens_kernel") == 4 and _n(counts, "packed_pos_rows_kernel") == 4
    assert bool(torch.isfinite(loss).all())
    assert not torch.equal(before, m.eeg_encoder.weight.detach())


def test_dpsgd_step_on_a_masked_window_batch():
    from eegfusion.dpsgd import GradSampleModule
    prefixes = ("bert.encoder.layer.11.", "bert.pooler.", "fc_layers.", "visual_encoder.", "classifier.")
    m = wc.build("concat")
    for n, q in m.named_parameters():
        q.requires_grad = n.startswith(prefixes)
    wm = GradSampleModule(m.cuda().train(), max_grad_norm=1e-3)
    (logits, grads), counts = _counts(lambda: wc.run(wm._module, "t256m", dev=DEV))
    # padded route: the dense attention kernels with the key bias, B * L rows
    assert _n(counts, "packed_pos_rows_kernel") == 0 and _n(counts, "window_patch_tokens_kernel") == 1
    clip = wm._module._dp["last_clip"].cpu()
    assert bool(torch.isfinite(clip).all()) and bool((clip > 0).all()) and bool((clip < 1).all())
    assert set(grads) == {n for n, q in m.named_parameters() if q.requires_grad}
    for n, g in grads.items():
        assert bool(torch.isfinite(g).all()), n
        if not n.endswith("attention.self.key.bias"):
            assert float(g.abs().max()) > 0, n
    # the clipped sum is bounded by B * C
    tot = sum(float((g ** 2).sum()) for g in grads.values()) ** 0.5
    assert tot <= 3 * 1e-3 * (1 + 1e-3)
