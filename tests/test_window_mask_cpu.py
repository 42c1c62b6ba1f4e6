"""Window contract at any length, with a step mask and a patch tokenizer, on the host path
(eegfusion/cpu_path.py) against the oracle: logits within 1e-5 and every parameter gradient within 1e-4,
both relative to the tensor's largest magnitude (the bounds of tests/test_host_path_cpu.py).  The cases
(tests/window_cases.py): T = 200 with prefix lengths [200, 137, 1]; the same with steps 50-89 of row 0
masked; eeg_patch 4 at T = 512 with partly valid last patches."""
import pytest
import torch
import torch.nn.functional as F

import window_cases as wc


@pytest.mark.parametrize("variant", ["concat", "prigumbel"])
@pytest.mark.parametrize("case", ["prefix", "hole", "patch4"])
def test_masked_window_host_vs_oracle(variant, case):
    m = wc.build(variant, wc.CASES[case]["P"])
    logits, grads = wc.run(m, case)
    wc.check(logits, grads, *wc.oracle(variant, case), 1e-5, 1e-4)


def test_cases_discriminate():
    """the masks matter: the oracle's logits with and without them differ by far more than the bounds"""
    bt = wc.batch("prefix")
    p = wc.params("concat", 1, False)
    pc = wc.O.PathConfig(contract="W", variant="concat")
    with torch.no_grad():
        full = wc.O.forward(p, dict(eeg=bt["eeg"], act=bt["act"]), pc)
    masked = wc.oracle("concat", "prefix")[0]
    holed = wc.oracle("concat", "hole")[0]
    assert wc.rel(full[0:1], masked[0:1]) < 1e-5              # row 0 is all valid
    assert wc.rel(full[1:], masked[1:]) > 1e-3
    assert wc.rel(holed[0:1], masked[0:1]) > 1e-3


def test_patch_embedding_is_conv1d():
    """eeg_encoder over patch rows = Conv1d(C, 768, kernel P, stride P) with weight.view(768, C, P)"""
    from eegfusion import cpu_path
    P, T = 4, 64
    m = wc.build("concat", P)
    g = torch.Generator().manual_seed(3)
    eeg = torch.randn(2, wc.C, T, generator=g)
    w, b = m.eeg_encoder.weight.detach(), m.eeg_encoder.bias.detach()
    assert tuple(w.shape) == (768, wc.C * P) and "eeg_encoder.weight" in m.state_dict()
    ref = F.conv1d(eeg, w.view(768, wc.C, P), b, stride=P).transpose(1, 2)        # [B, L, 768]
    seen = {}
    lin = cpu_path._lin

    def spy(x, mod):
        out = lin(x, mod)
        if mod is m.eeg_encoder:
            seen["x"] = out
        return out
    cpu_path._lin = spy
    try:
        with torch.no_grad():
            cpu_path._bert(m, m.engine.cfg, {"eeg": eeg}, training=False)
    finally:
        cpu_path._lin = lin
    assert float(ref.abs().max()) > 1.0
    assert float((seen["x"] - ref).abs().max()) < 2e-6


@pytest.mark.parametrize("patch, case", [(1, "hole"), (4, "patch4")])
def test_masked_steps_are_never_read(patch, case):
    """1e3 and NaN written into the masked steps give the logits of the clean window"""
    bt = wc.batch(case)
    m = wc.build("concat", patch).eval()
    dirty = bt["eeg"].clone()
    off = bt["mask"] == 0
    dirty[off[:, None, :].expand_as(dirty)] = 1e3
    dirty[:, ::2][off[:, None, :].expand_as(dirty[:, ::2])] = float("nan")
    with torch.no_grad():
        clean = m.forward_window(bt["eeg"], bt["act"], True, eeg_mask=bt["mask"])
        got = m.forward_window(dirty, bt["act"], True, eeg_mask=bt["mask"].bool())
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)


def test_all_ones_mask_is_no_mask():
    bt = wc.batch("prefix")
    m = wc.build("concat").eval()
    with torch.no_grad():
        a = m.forward_window(bt["eeg"], bt["act"])
        b = m.forward_window(bt["eeg"], bt["act"], eeg_mask=torch.ones(3, 200, dtype=torch.int32))
    assert torch.equal(a, b)


def test_v1_forward_window_takes_the_mask():
    import inspect
    from eegfusion.modules import FusionModel, PriGumbelV1Model
    for cls in (FusionModel, PriGumbelV1Model):
        assert "eeg_mask" in inspect.signature(cls.forward_window).parameters
    from eegfusion.engine import EngineConfig
    assert EngineConfig().eeg_patch == 1


def test_front_end_argument_errors_without_gpu():
    """the new entry points validate before any launch: EEGF_ERR_ARG, nothing enqueued"""
    from eegfusion import _lib
    lib = _lib.lib()
    assert lib.eegf_window_patch_tokens(0, 2, 64, 64, 3, None, None, 128, 128, None, None, None) == _lib.ERR_ARG
    assert lib.eegf_window_patch_tokens(0, 2, 129, 64, 1, None, None, 128, 128, None, None, None) == _lib.ERR_ARG
    assert lib.eegf_window_token_mask(2, 63, 2, None, None, None) == _lib.ERR_ARG
    assert lib.eegf_packed_pos_rows(2, 64, 768, None, 128, 128, None, None, None) == _lib.ERR_ARG


def test_refused_windows():
    """every refusal is a ValueError raised before anything is computed"""
    from eegfusion.modules import ConcatModel
    act = torch.zeros(2, wc.A)

    def model(patch=1, ch=wc.C):
        return ConcatModel(contract="W", dropout=0.0, eeg_patch=patch, eeg_channels=ch)

    def win(m, ch, T, mask=None):
        return m.forward_window(torch.zeros(2, ch, T), act, True, eeg_mask=mask)
    with pytest.raises(ValueError, match="multiple of eeg_patch"):
        win(model(4), wc.C, 202)                                   # T % P
    with pytest.raises(ValueError, match="position"):
        win(model(), wc.C, 1024)                                   # L > 512
    with pytest.raises(ValueError, match="position"):
        win(model(2), wc.C, 1026)
    for bad in (0, 3, 16):
        with pytest.raises(ValueError, match="eeg_patch"):
            win(model(bad), wc.C, 48)                              # P not in {1, 2, 4, 8}
    with pytest.raises(ValueError, match="1024"):
        win(model(8, 136), 136, 64)                                # C * P > 1024
    with pytest.raises(ValueError, match="multiple of 8"):
        win(model(2, 30), 30, 64)                                  # (C * P) % 8
    m = model()
    for shape in ((2, 100), (3, 200), (2, 1, 200), (200,)):
        with pytest.raises(ValueError, match="eeg_mask"):
            win(m, wc.C, 200, torch.ones(shape, dtype=torch.int64))
    empty = torch.ones(2, 200, dtype=torch.int64)
    empty[1] = 0
    with pytest.raises(ValueError, match="no valid token"):
        win(m, wc.C, 200, empty)
    # accepted now: any L <= 512 at P = 1, odd C at P = 1, L = 512 from T = 1024 at P = 2
    assert win(m, wc.C, 7).shape == (2, 2)
    assert win(model(1, 30), 30, 10).shape == (2, 2)
