"""GPU tests of the scalar end of the training step against the float64 references of tests/train_loss_cases.py:
sk_train_loss, sk_baked_embed_to_prob, sk_train_tversky, sk_train_cldice_term_field, sk_train_cldice_chain and
sk_train_adamw, each through skoots_amd._ffi and, where one exists, through its skoots_amd wrapper.

The cases reach what tests/golden/loss.npz (960 voxels, symmetric parameters) cannot: more than one partial row, the ragged
last row, the finalize kernels' second trip (more than 256 rows), the row cap, the second trip of the grid-stride loops,
anisotropic sigma / scale, unequal weights, a visible eps, empty and all-foreground samples, targets holding -1 and 0.5,
saturated logits, and AdamW with a weight decay that fp32 can see.  tests/test_train_loss_cases_cpu.py shows that the
bounds used here separate the kernels from every error the table was built for.

Bounds (train_loss_cases): losses max(2e-6, 4 d32), d32 the case's own fp32 CPU evaluation against float64; gradients 1e-4
of the reference's maximum per sample and logit channel, exactly 0 where the reference channel is identically 0;
probabilities rtol 1e-5 / atol 1e-7; AdamW max(4 d32, 4 fp32 ulps) per tensor.  Output buffers are NaN before every call
(what is not written shows), gradients carry a 1024-float guard.
"""
import numpy as np
import pytest
import torch

from tests import train_loss_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024
NAN = float("nan")


@pytest.fixture(scope="module")
def ffi():
    from skoots_amd import _ffi
    return _ffi


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _guarded(numel):
    """a NaN buffer of numel + GUARD floats -> (buffer, the numel floats a kernel may write, the guard behind them)"""
    buf = torch.full((numel + GUARD,), NAN, device=DEV)
    return buf, buf[:numel], buf[numel:]


def _device_inputs(case):
    d, B, n = K.inputs(case), case.B, K.voxels(case)
    return (d["logits"].contiguous().to(DEV), d["masks"].reshape(B, n).contiguous().to(DEV),
            d["skele"].reshape(B, n).contiguous().to(DEV), d["baked"].reshape(B, 3, n).contiguous().to(DEV))


def _run_loss(ffi, case, dev, need_grad=True):
    """sk_train_loss on NaN-filled outputs -> (losses (4,), dlogits (B, X, Y, Z, 5) or None), on the CPU"""
    lg, m, sk, bk = dev
    B, (X, Y, Z), n = case.B, case.shape, K.voxels(case)
    losses = torch.full((16,), NAN, device=DEV)
    ws = torch.full((int(ffi.lib.sk_train_loss_workspace_floats(B, n)),), NAN, device=DEV)
    buf, body, guard = _guarded(lg.numel()) if need_grad else (None, None, None)
    ffi.check(ffi.lib.sk_train_loss(ffi.ptr(lg), ffi.ptr(m), ffi.ptr(sk), ffi.ptr(bk), B, X, Y, Z, ffi.float_array(list(case.scale)),
                                    ffi.float_array(list(case.sigma)), ffi.float_array(K.loss_params(case)), ffi.ptr(losses),
                                    ffi.ptr(buf), ffi.ptr(ws), ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.current_stream().synchronize()
    if need_grad:
        assert torch.isnan(guard).all(), "sk_train_loss wrote behind dlogits"
        return losses[:4].cpu(), body.reshape(lg.shape).cpu()
    return losses[:4].cpu(), None


# ---------------------------------------------------------------------------------------------- sk_train_loss
@pytest.mark.parametrize("name", K.NAMES)
def test_fused_loss_vs_float64(ffi, name):
    """Losses and d total / d logits on every case; the same bits without a gradient, on a second run, on a side stream and
    through skoots_amd.train.fused_loss.  Measured on the MI355X: d32 2.6e-8 ... 1.4e-7 (the bound is 2e-6 on every case),
    losses at most 9.7e-8 from float64, gradients at most 2.3e-6 of a channel's maximum (at the two largest cases, 4e-7
    below them)."""
    from skoots_amd.train import fused_loss
    case = K.BY_NAME[name]
    ref, dev = K.loss64(case), _device_inputs(case)
    losses, dl = _run_loss(ffi, case, dev)
    err = (losses.double() - ref["losses"]).abs().max().item()
    bad, worst = K.grad_violations(dl, ref["grad"])
    print(f"MEASURED {name}: d32 {K.loss_d32(case):.2e} bound {K.loss_bound(case):.2e} losses off by {err:.2e}; "
          f"gradient off by {worst:.2e} of a channel's maximum")
    assert torch.isfinite(losses).all() and torch.isfinite(dl).all()
    assert err <= K.loss_bound(case), (losses.tolist(), ref["losses"].tolist())
    assert not bad, bad
    if case.kind == "edges":
        for b, x, y, z, c, v in K.PLANTED:
            g = dl[b, x, y, z, c].item()
            assert g == 0.0 if (b, x, y, z, c, v) in K.PLANTED_ZERO else abs(g) < 1e-15, (b, x, y, z, c, v, g)
    # value only: dlogits = NULL
    l0, none = _run_loss(ffi, case, dev, need_grad=False)
    assert none is None and _same_bits(l0, losses)
    # deterministic, and independent of the stream
    l1, d1 = _run_loss(ffi, case, dev)
    assert _same_bits(l1, losses) and _same_bits(d1, dl)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        l2, d2 = _run_loss(ffi, case, dev)
    torch.cuda.synchronize()
    assert _same_bits(l2, losses) and _same_bits(d2, dl)
    # the wrapper: masks / skeleton (B, 1, X, Y, Z), baked (B, 3, X, Y, Z)
    d = K.inputs(case)
    l3, d3 = fused_loss(dev[0], d["masks"].to(DEV), d["skele"].to(DEV), d["baked"].to(DEV), list(case.sigma), list(case.scale),
                        [tuple(t) for t in case.triples], list(case.weights))
    assert _same_bits(l3.cpu(), losses) and _same_bits(d3.cpu(), dl)
    l4, d4 = fused_loss(dev[0], d["masks"].to(DEV), d["skele"].to(DEV), d["baked"].to(DEV), list(case.sigma), list(case.scale),
                        [tuple(t) for t in case.triples], list(case.weights), need_grad=False)
    assert d4 is None and _same_bits(l4.cpu(), losses)


# ---------------------------------------------------------------------------------------------- sk_baked_embed_to_prob
@pytest.mark.parametrize("eps", [1e-16, 0.5])
@pytest.mark.parametrize("n", K.EMBED_PROB_SIZES)
def test_embed_prob_vs_float64(ffi, n, eps):
    """B = 3, sigma (20, 10, 5); eps = 0.5 because the default 1e-16 vanishes in fp32 (the CPU test shows that 0.5 moves the
    result by more than 1 %).  The last size takes the grid-stride loop's second trip."""
    from skoots_amd.lib.embedding_to_prob import baked_embed_to_prob
    emb, baked = K.embed_prob_inputs(n)
    want = K.embed_prob64(emb, baked, K.SIGMA, eps)
    e, s = torch.tensor(emb).to(DEV), torch.tensor(baked).to(DEV)
    buf, body, guard = _guarded(3 * n)
    ffi.check(ffi.lib.sk_baked_embed_to_prob(ffi.ptr(e), ffi.ptr(s), ffi.ptr(buf), 3, n, ffi.float_array(list(K.SIGMA)), eps,
                                             ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert torch.isnan(guard).all()
    got = body.reshape(3, n).cpu()
    ratio = K.prob_violation(got, want)
    print(f"MEASURED embed_prob n {n} eps {eps}: {ratio:.3f} of the bound")
    assert ratio <= 1.0
    wrapped = baked_embed_to_prob(e.reshape(3, 3, n, 1, 1), s.reshape(3, 3, n, 1, 1), list(K.SIGMA), eps)
    assert wrapped.shape == (3, 1, n, 1, 1) and _same_bits(wrapped.reshape(3, n).cpu(), got)


# ---------------------------------------------------------------------------------------------- sk_train_tversky
@pytest.mark.parametrize("kind", ["binary", "ids", "empty-middle", "cap"])
def test_tversky_vs_float64(ffi, kind):
    """Binary ground truth: the float64 sums, which on such a ground truth are oracle.train_step.tversky (CPU test).  "ids":
    the header's rule, every non-zero value (ids, -1, 0.5) one foreground -- NOT the reference, which expands per id.
    "empty-middle": B = 3, the middle sample takes the constant.  "cap": 4096 * 4096 + 4097 voxels, beyond the row cap.
    Bound max(2e-6, 4 d32), d32 from numpy's fp32 sums."""
    from skoots_amd.train import tversky
    pred, gt = K.tversky_inputs(kind)
    B, n = pred.shape
    p, g = torch.tensor(pred).to(DEV), torch.tensor(gt).to(DEV)
    for alpha, beta, eps in (K.TRIPLES if kind != "cap" else K.TRIPLES[:1]):
        want = K.tversky64(pred, gt, alpha, beta, eps)
        bound = max(K.LOSS_ATOL, 4 * abs(K.tversky64(pred, gt, alpha, beta, eps, dtype=np.float32) - want))
        loss = torch.full((1,), NAN, device=DEV)
        ws = torch.full((int(ffi.lib.sk_train_loss_workspace_floats(B, n)),), NAN, device=DEV)
        ffi.check(ffi.lib.sk_train_tversky(ffi.ptr(p), ffi.ptr(g), B, n, alpha, beta, eps, ffi.ptr(loss), ffi.ptr(ws),
                                           ffi.stream_ptr(torch.device(DEV))))
        got = loss.cpu()
        print(f"MEASURED tversky {kind} {(alpha, beta, eps)}: off by {abs(got.item() - want):.2e}, bound {bound:.2e}")
        assert abs(got.item() - want) <= bound, (got.item(), want)
        wrapped = tversky(alpha, beta, eps)(p.reshape(B, 1, n, 1, 1), g.reshape(B, 1, n, 1, 1))
        assert _same_bits(wrapped.reshape(1).cpu(), got)


# ---------------------------------------------------------------------------------------------- soft-clDice term plumbing
FIELD_CASES = [c.name for c, _ in K.TABLE] + ["7x11x13-edges"]
CHAIN_CASES = ["1x1x1", "3x5x7", "7x11x13", "7x11x13-edges", "17x16x16", "67x129x127"]


def _term_call(ffi, case, dev, term, with_baked=True):
    lg, m, sk, bk = dev
    B, (X, Y, Z), n = case.B, case.shape, K.voxels(case)
    pbuf, prob, pguard = _guarded(B * n)
    gbuf, gt, gguard = _guarded(B * n)
    ffi.check(ffi.lib.sk_train_cldice_term_field(ffi.ptr(lg), ffi.ptr(sk if term == 2 else m), ffi.ptr(bk if with_baked else None),
                                                 B, X, Y, Z, ffi.float_array(list(case.scale)), ffi.float_array(list(case.sigma)),
                                                 term, ffi.ptr(pbuf), ffi.ptr(gbuf), ffi.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert torch.isnan(pguard).all() and torch.isnan(gguard).all()
    return prob.reshape(B, n).cpu(), gt.reshape(B, n).cpu()


@pytest.mark.parametrize("term", [0, 1, 2])
@pytest.mark.parametrize("name", FIELD_CASES)
def test_cldice_term_field_vs_float64(ffi, name, term):
    """prob against float64 (term 0 the embedding probability, 1 sigmoid(l[4]), 2 sigmoid(l[3])), gt exactly target > 0 (the
    edges case holds -1 and 0.5); baked = NULL gives the same bits for terms 1 and 2 and is refused for term 0."""
    case = K.BY_NAME[name]
    dev = _device_inputs(case)
    want_p, want_g = K.term_field64(case, term)
    prob, gt = _term_call(ffi, case, dev, term)
    ratio = K.prob_violation(prob, want_p)
    print(f"MEASURED term_field {name} term {term}: {ratio:.3f} of the bound")
    assert ratio <= 1.0
    assert torch.equal(gt, want_g)
    if term:
        p2, g2 = _term_call(ffi, case, dev, term, with_baked=False)
        assert _same_bits(p2, prob) and _same_bits(g2, gt)
    else:
        with pytest.raises(ValueError):
            _term_call(ffi, case, dev, term, with_baked=False)


@pytest.mark.parametrize("term", [0, 1, 2])
@pytest.mark.parametrize("name", CHAIN_CASES)
def test_cldice_chain_vs_float64(ffi, name, term):
    """On random dprob and term_loss, with dlogits and losses holding random values: the term's channels become prefill +
    weight dprob d prob / d logits (bound: GRAD_REL of the increment's maximum per sample and channel, plus the one fp32
    rounding of the stored sum, 2^-23 of it), the other channels keep their bits; losses[term] = term_loss, losses[3]
    grows by weight term_loss (two fp32 roundings: 2^-23 (|losses[3]| + |weight term_loss|)), the other twelve entries
    keep their bits.  With dprob = dlogits = NULL only the losses change."""
    case = K.BY_NAME[name]
    lg, m, sk, bk = _device_inputs(case)
    B, (X, Y, Z), n = case.B, case.shape, K.voxels(case)
    gen = torch.Generator().manual_seed(500 + term)
    dprob = torch.randn((B, n), generator=gen)
    prefill = torch.randn((B, X, Y, Z, 5), generator=gen)
    losses0 = torch.randn(16, generator=gen)
    term_loss, weight = torch.tensor([0.6180339887]), (1.0, 2.0, 0.5)[term]
    inc = K.chain64(case, term, weight, dprob)
    dprob_d, term_loss_d = dprob.to(DEV), term_loss.to(DEV)

    def call(grad):
        buf, body, guard = _guarded(prefill.numel())
        body.copy_(prefill.reshape(-1))
        losses = losses0.to(DEV)
        ffi.check(ffi.lib.sk_train_cldice_chain(ffi.ptr(lg), ffi.ptr(bk), B, X, Y, Z, ffi.float_array(list(case.scale)),
                                                ffi.float_array(list(case.sigma)), term, weight,
                                                ffi.ptr(dprob_d) if grad else None, ffi.ptr(term_loss_d),
                                                ffi.ptr(losses), ffi.ptr(buf) if grad else None,
                                                ffi.stream_ptr(torch.device(DEV))))
        torch.cuda.synchronize()
        assert torch.isnan(guard).all()
        return losses.cpu(), body.reshape(prefill.shape).cpu()

    for grad in (True, False):
        losses, dl = call(grad)
        mine = [0, 1, 2] if term == 0 else [4 if term == 1 else 3]
        others = [c for c in range(5) if c not in mine]
        assert _same_bits(dl[..., others], prefill[..., others])
        if grad:
            want = prefill.double() + inc
            top = inc.abs().reshape(B, -1, 5).amax(dim=1).reshape(B, 1, 1, 1, 5)
            tol = K.GRAD_REL * top + 2.0 ** -23 * want.abs()
            ratio = ((dl.double() - want).abs()[..., mine] / tol[..., mine].clamp_min(1e-300)).max().item()
            print(f"MEASURED chain {name} term {term}: {ratio:.3f} of the bound")
            assert (inc[..., others] == 0).all() and top[..., mine].min().item() > 0
            assert ratio <= 1.0
        else:
            assert _same_bits(dl, prefill)
        keep = [i for i in range(16) if i not in (term, 3)]
        assert _same_bits(losses[keep], losses0[keep]) and _same_bits(losses[term:term + 1], term_loss)
        want3 = losses0[3].double().item() + K.r32(weight) * term_loss.double().item()
        assert abs(losses[3].item() - want3) <= 2.0 ** -23 * (abs(losses0[3].item()) + abs(weight * term_loss.item()))


# ---------------------------------------------------------------------------------------------- sk_train_adamw
def _adamw(ffi, p, g, m, v, n, params, step):
    lr, b1, b2, eps, wd = K.ADAMW_PARAMS[params]
    return ffi.lib.sk_train_adamw(ffi.ptr(p), ffi.ptr(g), ffi.ptr(m), ffi.ptr(v), n, lr, b1, b2, eps, wd, step,
                                  ffi.stream_ptr(torch.device(DEV)))


@pytest.mark.parametrize("params", sorted(K.ADAMW_PARAMS))
@pytest.mark.parametrize("n", K.ADAMW_SIZES)
def test_adamw_vs_float64(ffi, n, params):
    """param, exp_avg and exp_avg_sq after steps 1, 2, 3 (carried) and step 1000 on the carried state against adamw_ref in
    float64, gradients spanning eight decades with exact zeros.  Bound per tensor and element: max(4 d32, 4 fp32 ulps of
    the reference value), d32 = the fp32 CPU evaluation's largest distance from float64 on the same inputs.  Measured d32
    at n = 2,097,665, largest over the four steps: "strong" (lr 1e-2, wd 0.1, betas (0.8, 0.95), eps 1e-3) p 1.08e-6,
    m 6.7e-8, v 1.2e-7; "defaults" p 7.1e-7, m 4.8e-8, v 1.7e-9; at n = 1: p 1.9e-8, m 1.2e-12, v 3.5e-17 (the ulp floor
    decides there).  The buffers carry a guard: n = 2,097,665 leaves a ragged last block on the loop's second trip."""
    p0, grads = K.adamw_inputs(n)
    bufs = [_guarded(n) for _ in range(3)]
    p, m, v = (b[1] for b in bufs)
    p.copy_(p0)
    m.zero_()
    v.zero_()
    refs, bounds = K.adamw_run(n, params), K.adamw_bounds(n, params)
    worst = [0.0, 0.0, 0.0]
    grads_d = grads.to(DEV)
    for i, step in enumerate(K.ADAMW_STEPS):
        ffi.check(_adamw(ffi, p, grads_d[i], m, v, n, params, step))
        for k, (got, want, (_, tol)) in enumerate(zip((p, m, v), refs[i], bounds[i])):
            ratio = ((got.cpu().double() - want).abs() / tol).max().item()
            worst[k] = max(worst[k], ratio)
            assert ratio <= 1.0, (("param", "exp_avg", "exp_avg_sq")[k], step, ratio)
    assert all(torch.isnan(b[2]).all() for b in bufs)
    zeros = (grads == 0).all(dim=0)
    assert (v.cpu()[zeros] == 0).all() and (m.cpu()[zeros] == 0).all()
    print(f"MEASURED adamw n {n} {params}: p, m, v at {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f} of their bounds")


def test_adamw_of_nothing_touches_nothing(ffi):
    gen = torch.Generator().manual_seed(3)
    host = [torch.randn(8, generator=gen) for _ in range(4)]
    dev = [t.to(DEV) for t in host]
    assert _adamw(ffi, dev[0], dev[1], dev[2], dev[3], 0, "strong", 1) == 0        # SK_OK
    torch.cuda.synchronize()
    assert all(_same_bits(d.cpu(), h) for d, h in zip(dev, host))
