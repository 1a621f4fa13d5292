"""The cases, seeded inputs and float64 references that tests/test_train_loss_cases_cpu.py and tests/test_hip_train_loss.py
share (torch and numpy on the CPU only): the scalar end of the training step -- sk_train_loss, sk_train_tversky,
sk_baked_embed_to_prob, sk_train_cldice_term_field, sk_train_cldice_chain (skoots_amd/csrc/train.hip, cldice.hip) and
sk_train_adamw.

The references are written from the definitions in include/skoots_hip.h and oracle/train_step.py, never from the kernels:

    E   = index + tanh(l[0:3]) * scale                       index = the voxel's (x, y, z)
    pe  = exp(sum_k (E_k - S_k)^2 / (-2 (sigma_k + 1e-16)^2))  S = baked
    ps  = sigmoid(l[3]) (skeleton),  pp = sigmoid(l[4]) (probability)
    per sample and term, with g the term's target as 0 / 1 (masks > 0 for pe and pp, skeleton > 0 for ps):
        TP = sum p g, FP = sum p (1 - g), FN = sum (1 - p) g
        1 - (TP + eps) / (TP + alpha (FP + 1e-10) + beta FN + eps)     when the sample has foreground,
        1 - eps / (alpha 1e-10 + eps)                                  when it has none (the reference's empty mask stack)
    term = batch mean; total = sum_k weight_k term_k; the gradient is float64 autograd of the total.

Every reference takes a ``mut`` naming ONE deliberate error (MUTATIONS / ADAMW_MUTATIONS); tests/test_train_loss_cases_cpu.py
shows that each of them leaves the bounds of the GPU test by a factor of 10 on some case, which is what makes those bounds
mean something.

Inputs are fp32 tensors, so the kernel and the reference read the same numbers; host parameters (sigma, scale, the
(alpha, beta, eps) triples, the weights, AdamW's hyperparameters) reach the library as C floats, so the references use
their fp32 roundings as well -- 1 - beta2 is then exact in both.

A case is ``Case(name, B, shape, sigma, scale, weights, triples, kind)``.  ``kind``:
    "plain"   ids 1..4 at density 0.4, skeleton density 0.1, logits 1.5 randn
    "edges"   B = 3.  Sample 0 plain with -1 and 0.5 planted in both targets (> 0 and != 0 disagree on -1) and +-40 planted
              in the logits (PLANTED); sample 1 has no instance but skeleton voxels, sample 2 instances but no skeleton:
              the two foreground counts are separate sums
    "allfg"   sample 0 is foreground everywhere in both targets: FP = 0, only the 1e-10 remains of that term
    "one"     the single voxel is an instance and not a skeleton: a full term and the empty-sample constant at n = 1
``baked`` is aimed at the embedding, E + sigma randn (0.6 on foreground, 2.5 on background), so that pe spans (0, 1)
(mean about 0.28) and the loss feels sigma and scale; a uniform baked leaves pe near 0.02 whatever the parameters.
"""
import collections
import functools

import numpy as np
import torch

Case = collections.namedtuple("Case", "name B shape sigma scale weights triples kind")

SIGMA, SCALE, WEIGHTS = (20.0, 10.0, 5.0), (60.0, 30.0, 12.0), (1.0, 2.0, 0.5)
TRIPLES = ((0.3, 0.7, 1e-2), (0.6, 0.4, 1e-8), (0.2, 1.8, 1e-4))
# the reference's defaults (skoots/config.py:49-64)
DEF_SIGMA, DEF_SCALE, DEF_WEIGHTS = (20.0, 20.0, 20.0), (60.0, 60.0, 12.0), (1.0, 1.0, 1.0)
DEF_TRIPLES = ((0.25, 0.75, 1e-8), (0.5, 0.5, 1e-8), (0.5, 1.5, 1e-8))


def _case(name, B, shape, kind="plain", sigma=SIGMA, scale=SCALE, weights=WEIGHTS, triples=TRIPLES):
    return Case(name, B, shape, sigma, scale, weights, triples, kind)


# (case, rows = sk_train_loss_num_blocks(voxels)): 4096 voxels per row
TABLE = [
    (_case("1x1x1", 1, (1, 1, 1), "one", DEF_SIGMA, DEF_SCALE, DEF_WEIGHTS, DEF_TRIPLES), 1),  # n = 1
    (_case("3x5x7", 2, (3, 5, 7)), 1),             # 105 voxels: fewer than a block's threads
    (_case("7x11x13", 3, (7, 11, 13)), 1),         # 1001 voxels, extents pairwise distinct: a wrong decode shows; B = 3
    (_case("16x16x16", 2, (16, 16, 16)), 1),       # exactly 4096 voxels: one full row
    (_case("17x16x16", 2, (17, 16, 16)), 2),       # 4352 voxels: two rows, the second ragged
    (_case("67x129x127", 2, (67, 129, 127)), 268),  # 1,097,661 voxels: more than 256 rows, the finalize loop's second trip
    (_case("129x127x131", 1, (129, 127, 131)), 524),  # 2,146,173 voxels > 4096 * 512: second trip of loss_bwd_kernel
]
VARIANTS = [
    _case("7x11x13-defaults", 3, (7, 11, 13), "plain", DEF_SIGMA, DEF_SCALE, DEF_WEIGHTS, DEF_TRIPLES),
    _case("7x11x13-w010", 3, (7, 11, 13), weights=(0.0, 1.0, 0.0)),
    _case("7x11x13-edges", 3, (7, 11, 13), "edges"),
    _case("7x11x13-allfg", 3, (7, 11, 13), "allfg"),
]
CASES = [c for c, _ in TABLE] + VARIANTS
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
SMALL = [c.name for c in CASES if c.shape[0] * c.shape[1] * c.shape[2] <= 4352]

CAP_VOXELS = 4096 * 4096 + 4097      # sk_train_tversky only: beyond the 4096-row cap, every row strides twice or more
EMBED_PROB_SIZES = (1, 255, 257, 2146173)
ADAMW_SIZES = (1, 255, 256, 257, 10007, 2097665)   # the last > 4096 * 512: the grid-stride loop's second trip
ADAMW_STEPS = (1, 2, 3, 1000)                       # carried state; 1000 runs on what step 3 left
ADAMW_PARAMS = {                                    # lr, beta1, beta2, eps, weight_decay
    "strong": (1e-2, 0.8, 0.95, 1e-3, 0.1),         # 1 - lr * wd != 1 in fp32, eps visible
    "defaults": (5e-4, 0.9, 0.999, 1e-8, 1e-6),     # the reference's; beta2^1000 = 0.37: the bias correction still matters
}

# (sample, x, y, z, channel, value) planted in the logits of an "edges" case.  tanh(+-40) is 1 to the last bit in float64
# and fp32, and so is sigmoid(40): the derivative there is exactly 0.  sigmoid(-40) = 4.2e-18 is representable in both, so
# the derivative at a -40 skeleton / probability logit is about 4e-18 times the coefficient: not 0, far below any bound.
PLANTED = [(0, 1, 2, 3, 0, 40.0), (0, 1, 2, 4, 1, -40.0), (0, 2, 3, 5, 2, 40.0), (0, 3, 1, 2, 0, -40.0),
           (0, 3, 1, 2, 3, 40.0), (0, 3, 1, 3, 4, 40.0), (0, 4, 1, 2, 3, -40.0), (0, 4, 1, 3, 4, -40.0)]
PLANTED_ZERO = [p for p in PLANTED if p[4] < 3 or p[5] > 0]

LOSS_ATOL = 2e-6      # test_fused_loss_vs_reference_golden's bound on the same four numbers
LOSS_D32_MAX = 5e-6   # a case whose own fp32 evaluation is further than this from float64 is badly conditioned
GRAD_REL = 1e-4       # test_hip_train._close's bound, applied per sample and logit channel
PROB_RTOL, PROB_ATOL = 1e-5, 1e-7   # test_standalone_loss_functions' bound on the embedding probability

MUTATIONS = ("sigma_xy", "scale_xy", "decode_xy", "no_1e10", "no_eps", "weight_not_div_B", "prob_skel", "ne0", "empty0")
ADAMW_MUTATIONS = ("no_decay", "eps_in_sqrt", "no_bias_correction_1000")


def r32(x):
    """a host parameter as the library receives it: rounded to a C float"""
    return float(np.float32(x))


def voxels(case):
    return case.shape[0] * case.shape[1] * case.shape[2]


def loss_params(case):
    """loss_params_host of sk_train_loss: (3, 4) = alpha, beta, eps, weight"""
    return [v for t, w in zip(case.triples, case.weights) for v in (*t, w)]


# ---------------------------------------------------------------------------------------------- fields and loss
def _index(X, Y, Z, swapped=False):
    i = torch.arange(X * Y * Z)
    z, t = i % Z, i // Z
    x, y = (t % Y, t // Y) if swapped else (t // Y, t % Y)
    return torch.stack([x, y, z], dim=-1).reshape(X, Y, Z, 3)


def _fields(logits, baked, sigma, scale, mut=None):
    """(pe, ps, pp), each (B, X, Y, Z), in the dtype of ``logits`` (B, X, Y, Z, 5); differentiable"""
    dt = logits.dtype
    _, X, Y, Z, _ = logits.shape
    sg = torch.tensor([r32(s) for s in sigma], dtype=dt)
    sc = torch.tensor([r32(s) for s in scale], dtype=dt)
    if mut == "sigma_xy":
        sg = sg[[1, 0, 2]]
    if mut == "scale_xy":
        sc = sc[[1, 0, 2]]
    E = _index(X, Y, Z, mut == "decode_xy").to(dt) + torch.tanh(logits[..., 0:3]) * sc
    S = baked.to(dt).permute(0, 2, 3, 4, 1)
    pe = torch.exp(((E - S) ** 2 / (-2 * (sg + 1e-16) ** 2)).sum(dim=-1))
    cs, cp = (4, 3) if mut == "prob_skel" else (3, 4)
    return pe, torch.sigmoid(logits[..., cs]), torch.sigmoid(logits[..., cp])


def _tversky_per_sample(p, g, alpha, beta, eps, mut=None):
    """p, g (B, n) -> (B,) losses"""
    alpha, beta = r32(alpha), r32(beta)
    eps = 0.0 if mut == "no_eps" else r32(eps)
    tiny = 0.0 if mut == "no_1e10" else 1e-10
    tp, fp, fn = (p * g).sum(dim=1), (p * (1 - g)).sum(dim=1), ((1 - p) * g).sum(dim=1)
    full = 1 - (tp + eps) / (tp + alpha * (fp + tiny) + beta * fn + eps)
    empty = 0.0 if mut == "empty0" else 1 - eps / (alpha * tiny + eps)
    return torch.where(g.sum(dim=1) > 0, full, torch.full_like(full, empty))


def loss_ref(logits, masks, skele, baked, sigma, scale, triples, weights, dtype=torch.float64, mut=None, grad=True):
    """The fused loss of ``logits`` (B, X, Y, Z, 5), ``masks`` / ``skele`` (B, 1, X, Y, Z), ``baked`` (B, 3, X, Y, Z),
    evaluated in ``dtype``.  -> dict: losses (4,) float64 = embed, prob, skeleton, total; grad (B, X, Y, Z, 5) float64 =
    d total / d logits; pe, ps, pp (B, X, Y, Z)."""
    lg = logits.detach().to(dtype).clone().requires_grad_(grad)
    B = lg.shape[0]
    pe, ps, pp = _fields(lg, baked, sigma, scale, mut)
    fg = (lambda t: t != 0) if mut == "ne0" else (lambda t: t > 0)
    g, gs = fg(masks).to(dtype).reshape(B, -1), fg(skele).to(dtype).reshape(B, -1)
    per = [_tversky_per_sample(p.reshape(B, -1), t, *tr, mut=mut)
           for p, t, tr in ((pe, g, triples[0]), (pp, g, triples[1]), (ps, gs, triples[2]))]
    w = [r32(v) for v in weights]
    terms = [q.mean() for q in per]
    total = w[0] * terms[0] + w[1] * terms[1] + w[2] * terms[2]
    out = {"losses": torch.stack(terms + [total]).detach().double(), "pe": pe.detach(), "ps": ps.detach(), "pp": pp.detach()}
    if grad:
        obj = total if mut != "weight_not_div_B" else w[0] * per[0].sum() + w[1] * per[1].sum() + w[2] * per[2].sum()
        obj.backward()
        out["grad"] = lg.grad.double()
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> dict of fp32 tensors logits (B, X, Y, Z, 5), masks, skele (B, 1, X, Y, Z), baked (B, 3, X, Y, Z).  Shared and
    cached: never modified by a test."""
    B, (X, Y, Z) = case.B, case.shape
    gen = torch.Generator().manual_seed(1000 + NAMES.index(case.name))
    logits = 1.5 * torch.randn((B, X, Y, Z, 5), generator=gen)
    masks = (torch.rand((B, 1, X, Y, Z), generator=gen) < 0.4).float() * torch.randint(1, 5, (B, 1, X, Y, Z), generator=gen)
    skele = (torch.rand((B, 1, X, Y, Z), generator=gen) < 0.1).float()
    if case.kind == "one":
        masks.fill_(3.0)
        skele.zero_()
    elif case.kind == "allfg":
        masks[0] = torch.randint(1, 5, (1, X, Y, Z), generator=gen).float()
        skele[0] = 1.0
    elif case.kind == "edges":
        for t, count in ((masks, 24), (skele, 12)):
            flat = t[0].reshape(-1)
            pos = torch.randperm(flat.numel(), generator=gen)[:2 * count]
            flat[pos[:count]] = -1.0
            flat[pos[count:]] = 0.5
        masks[1] = 0.0
        skele[2] = 0.0
        assert (skele[1] > 0).any() and (masks[2] > 0).any()
        for b, x, y, z, c, v in PLANTED:
            logits[b, x, y, z, c] = v
    sg = torch.tensor(case.sigma, dtype=torch.float64).view(1, 3, 1, 1, 1)
    sc = torch.tensor(case.scale, dtype=torch.float64)
    E = (_index(X, Y, Z).double() + torch.tanh(logits[..., 0:3].double()) * sc).permute(0, 4, 1, 2, 3)
    spread = torch.where(masks > 0, 0.6, 2.5).double()
    baked = (E + sg * torch.randn((B, 3, X, Y, Z), generator=gen).double() * spread).float().contiguous()
    return {"logits": logits, "masks": masks, "skele": skele, "baked": baked}


def _loss_of(case, dtype, mut, grad):
    d = inputs(case)
    return loss_ref(d["logits"], d["masks"], d["skele"], d["baked"], case.sigma, case.scale, case.triples, case.weights,
                    dtype, mut, grad)


@functools.lru_cache(maxsize=None)
def loss64(case, mut=None):
    """the float64 reference of a case (see loss_ref), cached: read only"""
    return _loss_of(case, torch.float64, mut, True)


@functools.lru_cache(maxsize=None)
def loss_d32(case):
    """distance of the same formulas evaluated by torch in fp32 on the CPU from loss64, over the four losses"""
    return float((_loss_of(case, torch.float32, None, False)["losses"] - loss64(case)["losses"]).abs().max())


def loss_bound(case):
    """max(2e-6, 4 d32).  The factor 4 covers the kernel's different summation order: a thread adds at most 16 (17 at the
    cap size) terms in fp32, then 6 shuffles and 3 adds; the rest is double."""
    return max(LOSS_ATOL, 4 * loss_d32(case))


def grad_violations(got, ref):
    """``got``, ``ref`` (B, X, Y, Z, 5) -> list of (sample, channel, error / max |ref|) for every sample and logit channel
    that is further than GRAD_REL of that channel's own reference maximum; a channel whose reference is identically 0
    must be exactly 0 (reported as inf).  Also -> the largest ratio seen."""
    got, ref = got.double(), ref.double()
    bad, worst = [], 0.0
    for b in range(ref.shape[0]):
        for c in range(5):
            r, g = ref[b, ..., c], got[b, ..., c]
            top = float(r.abs().max())
            if top == 0.0:
                ratio = 0.0 if bool((g == 0).all()) else float("inf")
            else:
                ratio = float((g - r).abs().max()) / top
            worst = max(worst, ratio)
            if not ratio <= GRAD_REL:      # also catches NaN
                bad.append((b, c, ratio))
    return bad, worst


def prob_violation(got, ref):
    """largest |got - ref| / (PROB_ATOL + PROB_RTOL |ref|): <= 1 passes"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    r = ((got - ref).abs() / (PROB_ATOL + PROB_RTOL * ref.abs())).max()
    return float("inf") if bool(torch.isnan(r)) else float(r)


def term_field64(case, term, mut=None):
    """sk_train_cldice_term_field: (prob (B, n) float64, gt (B, n) fp32 = target > 0) of term 0 embed, 1 probability,
    2 skeleton"""
    ref, d = loss64(case, mut), inputs(case)
    prob = (ref["pe"], ref["pp"], ref["ps"])[term]
    target = d["skele"] if term == 2 else d["masks"]
    return prob.reshape(case.B, -1), (target > 0).float().reshape(case.B, -1)


def chain64(case, term, weight, dprob):
    """sk_train_cldice_chain's increment of dlogits: weight * dprob * d prob / d logits, (B, X, Y, Z, 5) float64, by
    autograd through the term's field.  ``dprob`` (B, n)."""
    d = inputs(case)
    lg = d["logits"].double().clone().requires_grad_(True)
    field = _fields(lg, d["baked"], case.sigma, case.scale)[(0, 2, 1)[term]]
    field.backward(r32(weight) * dprob.double().reshape(field.shape))
    return lg.grad


# ---------------------------------------------------------------------------------------------- stand-alone pieces
def embed_prob64(emb, baked, sigma, eps):
    """baked_embed_to_prob: emb, baked (B, 3, n) -> (B, n) float64"""
    sg = np.array([r32(s) for s in sigma], dtype=np.float64).reshape(1, 3, 1) + r32(eps)
    return np.exp((((np.asarray(emb, np.float64) - np.asarray(baked, np.float64)) ** 2) / (-2.0 * sg ** 2)).sum(axis=1))


@functools.lru_cache(maxsize=None)
def embed_prob_inputs(n, B=3):
    """-> emb, baked (B, 3, n) fp32 numpy, baked aimed at emb (one sigma of SIGMA away per axis on average)"""
    rng = np.random.default_rng(4000 + n % 1000)
    emb = (rng.random((B, 3, n)) * 150.0).astype(np.float32)
    baked = (emb + np.array(SIGMA).reshape(1, 3, 1) * rng.standard_normal((B, 3, n))).astype(np.float32)
    return emb, baked


def tversky64(pred, gt, alpha, beta, eps, dtype=np.float64, rule="ne0"):
    """sk_train_tversky by the header's rule: every non-zero value of gt (B, n) is ONE foreground; direct sums, no autograd"""
    alpha, beta, eps = r32(alpha), r32(beta), r32(eps)
    out = []
    for p, t in zip(np.asarray(pred), np.asarray(gt)):
        p = p.astype(dtype)
        g = ((t != 0) if rule == "ne0" else (t > 0)).astype(dtype)
        if g.sum() > 0:
            tp, fp, fn = (p * g).sum(), (p * (1 - g)).sum(), ((1 - p) * g).sum()
            out.append(1.0 - (float(tp) + eps) / (float(tp) + alpha * (float(fp) + 1e-10) + beta * float(fn) + eps))
        else:
            out.append(1.0 - eps / (alpha * 1e-10 + eps))
    return float(np.mean(out))


@functools.lru_cache(maxsize=None)
def tversky_inputs(kind):
    """-> pred, gt (B, n) fp32 numpy.  "binary": B 2, 1001 voxels; "ids": the same with ids 1..4, -1 and 0.5; "empty-middle":
    B 3, the middle sample without foreground; "cap": B 1, CAP_VOXELS."""
    rng = np.random.default_rng({"binary": 11, "ids": 12, "empty-middle": 13, "cap": 14}[kind])
    B, n = {"binary": (2, 1001), "ids": (2, 1001), "empty-middle": (3, 4352), "cap": (1, CAP_VOXELS)}[kind]
    pred = rng.random((B, n), dtype=np.float32)
    gt = (rng.random((B, n), dtype=np.float32) < 0.4).astype(np.float32)
    if kind == "ids":
        gt *= rng.integers(1, 5, (B, n)).astype(np.float32)
        gt[:, 5:400:17] = -1.0
        gt[:, 9:400:19] = 0.5
    if kind == "empty-middle":
        gt[1] = 0.0
    return pred, gt


# ---------------------------------------------------------------------------------------------- AdamW
def adamw_ref(p, g, m, v, lr, beta1, beta2, eps, wd, step, mut=None):
    """One decoupled-decay AdamW update (torch.optim.AdamW semantics) in the dtype of ``p`` -> (p, m, v):
    p <- p (1 - lr wd);  m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;
    p <- p - lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)."""
    dt = p.dtype
    lr, b1, b2, eps, wd = (torch.tensor(r32(x), dtype=dt) for x in (lr, beta1, beta2, eps, wd))
    one = torch.tensor(1.0, dtype=dt)
    if mut != "no_decay":
        p = p * (one - lr * wd)
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    bc1, bc2 = one - b1 ** step, one - b2 ** step
    if mut == "no_bias_correction_1000" and step >= 1000:
        bc1, bc2 = one, one
    denom = torch.sqrt(v / bc2 + eps) if mut == "eps_in_sqrt" else torch.sqrt(v) / torch.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


@functools.lru_cache(maxsize=None)
def adamw_inputs(n):
    """-> p0 (n,), grads (len(ADAMW_STEPS), n) fp32: randn * 10^U(-8, 0), with exact zeros planted at the same elements in
    every step (v stays 0 there and the denominator is eps alone)"""
    gen = torch.Generator().manual_seed(7000 + n % 1000)
    p0 = torch.randn(n, generator=gen)
    grads = torch.randn((len(ADAMW_STEPS), n), generator=gen) * 10.0 ** (-8.0 * torch.rand((len(ADAMW_STEPS), n), generator=gen))
    grads[:, 3::7] = 0.0
    return p0, grads


@functools.lru_cache(maxsize=None)
def adamw_run(n, params, dtype=torch.float64, mut=None):
    """the carried states after each of ADAMW_STEPS: list of (p, m, v) in ``dtype``; ``params`` a key of ADAMW_PARAMS"""
    p0, grads = adamw_inputs(n)
    p, m, v = p0.to(dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
    out = []
    for g, step in zip(grads, ADAMW_STEPS):
        p, m, v = adamw_ref(p, g.to(dtype), m, v, *ADAMW_PARAMS[params], step, mut)
        out.append((p, m, v))
    return out


def ulp32(x):
    """the fp32 unit in the last place at |x|, as float64"""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def adamw_bounds(n, params):
    """per step, per tensor (p, m, v): (d32, elementwise bound), d32 = the largest distance of the fp32 CPU evaluation from
    float64 and bound = max(4 d32, 4 fp32 ulps of the reference value)"""
    out = []
    for s64, s32 in zip(adamw_run(n, params), adamw_run(n, params, torch.float32)):
        row = []
        for r, e in zip(s64, s32):
            d = float((e.double() - r).abs().max())
            row.append((d, torch.maximum(torch.full_like(r, 4 * d), 4 * ulp32(r))))
        out.append(row)
    return out
