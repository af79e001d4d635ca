"""GPU: every calling form of the whole-model DiT pass at engine level -- the forward pass in one, two and three calls (sfron_dit_fwd.phase),
behind per-block events (block_ready), with the bf16 and the fp8 block GEMMs; the backward pass plain, data-parallel and with the factored
adaLN gradient.  The forms run the same kernels on the same operands in the same order: outputs and gradients are compared bit for bit.
Only Engine's public methods are called."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# 64 tokens, batch 4 -> M = 256: the smallest shape the fp8 tile takes (tests/test_gpu_fp8.py CFG); depth 2 gives block_ready a second entry
CFG = dict(input_size=16, patch_size=2, in_channels=4, hidden_size=128, depth=2, num_heads=2, num_classes=10)
B = 4
SENTINEL = 12345.0       # in the gradient arena before each backward pass: an element a form leaves unwritten differs from the plain pass (arena
                         # padding keeps it in every form, so it must compare equal to itself: not NaN)


class Case:
    """One engine with fixed inputs, and the plain forward + backward every other form is compared with."""

    def __init__(self, fp8):
        from oracle import dit_ref
        from sfron import dit
        torch.manual_seed(0)
        ref = dit_ref.DiT(**CFG)
        dit_ref.randomize_zero_init(ref, std=0.05, seed=1)
        self.model = dit.DiT(batch_size=B, **CFG)
        self.model.load_state_dict(ref.state_dict())
        self.eng = eng = self.model.engine
        if fp8:
            eng.enable_fp8()
        g = torch.Generator().manual_seed(3)
        S, Co = CFG["input_size"], 2 * CFG["in_channels"]
        self.x = torch.randn(B, CFG["in_channels"], S, S, generator=g).to(DEV)
        self.t = torch.tensor([5, 250, 600, 999], device=DEV)
        self.y = torch.tensor([1, 3, 5, 7], device=DEV)                      # distinct rows of the label table
        self.drop = torch.tensor([0, 1, 0, 0], dtype=torch.uint8, device=DEV)
        self.d_out = torch.randn(B, Co, S, S, generator=g).to(DEV)
        self.out, self.grads = self.forward_backward()

    def events(self):
        """depth already-recorded events and their handles, as Engine.dp_setup makes its own"""
        evs = [torch.cuda.Event(enable_timing=False) for _ in range(CFG["depth"])]
        for e in evs:
            e.record()
        return evs, (ctypes.c_void_p * len(evs))(*[e.cuda_event for e in evs])

    def forward(self, **kw):
        return self.eng.forward(self.x, self.t, self.y, self.drop, **kw).clone()

    def forward_backward(self, **kw):
        out = self.forward(**kw)
        self.eng.grads.fill_(SENTINEL)                                   # every trainable element is rewritten by the pass
        g = self.eng.backward(self.d_out, self.y, self.drop)
        torch.cuda.synchronize()
        return out, g[:self.eng.n_trainable].clone()

    def outside_ada_w(self, grads):
        lay, c = self.eng.layout, self.eng.cfg
        hi = lay["ada_w"] + (6 * c.depth + 2) * c.hidden * c.hidden
        return torch.cat([grads[:lay["ada_w"]], grads[hi:self.eng.n_trainable]])


@pytest.fixture(scope="module", params=["bf16", "fp8"])
def case(request):
    return Case(request.param == "fp8")


def test_plain_pass_is_finite_and_repeats_itself(case):
    assert torch.isfinite(case.out).all() and torch.isfinite(case.grads).all()
    for name, (off, shape, trainable) in case.eng.index.items():
        if trainable:                                                        # written, and not with zeros
            v = case.eng.view(case.grads, name)
            assert not (v == SENTINEL).any() and v.abs().max() > 0, name
    out, grads = case.forward_backward()
    assert torch.equal(out, case.out) and torch.equal(grads, case.grads)


@pytest.mark.parametrize("form", ["block_ready", "block_ready+between", "block_ready+ada_ready", "block_ready+between+ada_ready"])
def test_forward_forms_equal_the_plain_pass(case, form):
    evs, handles = case.events()
    calls = []
    kw = dict(block_ready=handles)
    if "between" in form:
        kw["between"] = lambda: calls.append(1)
    if "ada_ready" in form:
        kw["ada_ready"] = torch.cuda.Event(enable_timing=False)
        kw["ada_ready"].record()
    out, grads = case.forward_backward(**kw)
    assert len(calls) == (1 if "between" in form else 0)                     # exactly once per pass
    assert torch.equal(out, case.out)
    assert torch.equal(grads, case.grads)                                    # the backward pass reads every saved activation


def test_backward_forms(case):
    eng = case.eng
    case.forward()
    eng.grads.fill_(SENTINEL)
    g_dp = eng.backward_dp(case.d_out, case.y, case.drop)
    assert g_dp is eng.grads
    eng.scatter_late_bias()
    torch.cuda.synchronize()
    assert torch.equal(case.outside_ada_w(g_dp), case.outside_ada_w(case.grads))
    dmod_dp, sc_dp = eng.ada_dmod.clone(), eng.ada_sc.clone()

    case.forward()
    eng.grads.fill_(SENTINEL)
    r = eng.backward_factored_ada(case.d_out, case.y, case.drop)
    torch.cuda.synchronize()
    assert torch.equal(case.outside_ada_w(eng.grads), case.outside_ada_w(case.grads))
    assert r["lo"] == eng.layout["ada_w"] and r["NM"] == (6 * CFG["depth"] + 2) * CFG["hidden_size"] and r["D"] == CFG["hidden_size"] and r["R"] == B
    assert torch.equal(r["dmod"], dmod_dp) and torch.equal(r["sc"], sc_dp)
    assert dmod_dp.abs().max() > 0 and sc_dp.abs().max() > 0
