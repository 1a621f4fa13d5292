"""What makes the assertions of tests/test_hip_train_loss.py mean something, checked from the references of
tests/train_loss_cases.py and the library's host-only size queries alone (CPU).

The references: loss64 against the project's oracle (oracle/train_step.py, float64) and against tests/golden/loss.npz, the
reference's own numbers; adamw_ref against torch.optim.AdamW.  The table: the row counts and loop trips it claims, read
from sk_train_loss_num_blocks and sk_train_loss_workspace_floats.  The bounds: every case is well conditioned (its own fp32
evaluation within 5e-6 of float64), and every deliberate error of train_loss_cases.MUTATIONS / ADAMW_MUTATIONS leaves the
GPU test's bound on some quantity of some case by a factor of 10 -- if one did not, the cases would change, not the factor.
"""
import numpy as np
import pytest
import torch

from tests import train_loss_cases as K

FACTOR = 10.0


def _out(logits):
    """(B, X, Y, Z, 5) logits -> the model output (B, 5, X, Y, Z) the oracle's step_loss takes"""
    return torch.cat([torch.tanh(logits[..., 0:3]), torch.sigmoid(logits[..., 3:5])], dim=-1).permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("name", K.SMALL + ["67x129x127"])
def test_loss64_equals_the_oracle_in_float64(name):
    """oracle.train_step.step_loss + autograd, run in float64 on the same inputs (parameters as the C floats the library
    receives): losses and gradient to 1e-12."""
    from oracle import train_step as O
    case, d = K.BY_NAME[name], K.inputs(K.BY_NAME[name])
    lg = d["logits"].double().requires_grad_(True)
    tr = [tuple(K.r32(v) for v in t) for t in case.triples]
    want = O.step_loss(_out(lg), d["masks"], d["skele"], d["baked"].double(), torch.tensor(case.sigma, dtype=torch.float64),
                       torch.tensor(case.scale), *tr, weights=[K.r32(w) for w in case.weights])
    want[3].backward()
    ref = K.loss64(case)
    assert (torch.stack(want).detach() - ref["losses"]).abs().max().item() <= 1e-12
    assert (lg.grad - ref["grad"]).abs().max().item() <= 1e-12 * max(1.0, ref["grad"].abs().max().item())


def test_loss64_reproduces_the_golden_fixture(golden):
    """tests/golden/loss.npz (the reference's own tversky and baked_embed_to_prob) within the bounds the fixture's GPU test
    applies: losses 2e-6, gradient 1e-4 of its maximum, embedding probability rtol 1e-5 / atol 1e-7."""
    from tests.test_hip_train import _cf, _cl, _close, _golden_logits
    d = golden("loss.npz")
    logits, dact = _golden_logits(d)
    ref = K.loss_ref(_cl(logits), torch.tensor(d["masks"]), torch.tensor(d["skele"]), torch.tensor(d["baked"]),
                     d["sigma"].tolist(), d["scale"].tolist(), K.DEF_TRIPLES, K.DEF_WEIGHTS)
    np.testing.assert_allclose(ref["losses"].numpy(), d["losses"], rtol=0, atol=2e-6)
    _close(_cf(ref["grad"]), torch.tensor(d["grad"]).double() * dact, 1e-4, "d loss / d logits")
    np.testing.assert_allclose(ref["pe"].numpy(), d["embed_prob"][:, 0], rtol=1e-5, atol=1e-7)


def test_standalone_references_equal_the_oracle():
    """embed_prob64 and, on binary ground truth, tversky64 equal oracle.train_step's functions in float64.  On a ground
    truth with several ids they do NOT: the reference expands one mask per id, the port counts every non-zero value as one
    foreground (include/skoots_hip.h) -- which is why the reference's callers pass masks.gt(0)."""
    from oracle import train_step as O
    emb, baked = K.embed_prob_inputs(257)
    for eps in (1e-16, 0.5):
        want = O.baked_embed_to_prob(torch.tensor(emb).double().reshape(3, 3, 257, 1, 1),
                                     torch.tensor(baked).double().reshape(3, 3, 257, 1, 1),
                                     torch.tensor(K.SIGMA, dtype=torch.float64), K.r32(eps))
        assert np.abs(K.embed_prob64(emb, baked, K.SIGMA, eps) - want.reshape(3, 257).numpy()).max() <= 1e-14
    assert np.abs(K.embed_prob64(emb, baked, K.SIGMA, 0.5) / K.embed_prob64(emb, baked, K.SIGMA, 1e-16) - 1).max() > 0.01

    def oracle(kind, tr):
        pred, gt = K.tversky_inputs(kind)
        B, n = pred.shape
        return O.tversky(torch.tensor(pred).double().reshape(B, 1, n, 1, 1), torch.tensor(gt).reshape(B, 1, n, 1, 1),
                         *(K.r32(v) for v in tr)).item()
    for tr in K.TRIPLES + K.DEF_TRIPLES:
        for kind in ("binary", "empty-middle"):
            assert abs(K.tversky64(*K.tversky_inputs(kind), *tr) - oracle(kind, tr)) <= 1e-12
    assert abs(K.tversky64(*K.tversky_inputs("ids"), *K.TRIPLES[0]) - oracle("ids", K.TRIPLES[0])) > 1e-2
    # and the two foreground rules differ on that ground truth (-1 is foreground for != 0 only)
    pred, gt = K.tversky_inputs("ids")
    assert abs(K.tversky64(pred, gt, *K.TRIPLES[0]) - K.tversky64(pred, gt, *K.TRIPLES[0], rule="gt0")) > 10 * K.LOSS_ATOL


@pytest.mark.parametrize("params", sorted(K.ADAMW_PARAMS))
def test_adamw_ref_equals_torch_adamw_in_float64(params):
    lr, b1, b2, eps, wd = (K.r32(v) for v in K.ADAMW_PARAMS[params])
    p0, grads = K.adamw_inputs(10007)
    p = torch.nn.Parameter(p0.double())
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    q, m, v = p0.double(), torch.zeros(10007, dtype=torch.float64), torch.zeros(10007, dtype=torch.float64)
    for step in (1, 2, 3):
        p.grad = grads[step - 1].double()
        opt.step()
        q, m, v = K.adamw_ref(q, grads[step - 1].double(), m, v, *K.ADAMW_PARAMS[params], step)
        st = opt.state[p]
        assert (q - p.detach()).abs().max().item() <= 1e-14
        assert (m - st["exp_avg"]).abs().max().item() <= 1e-14 and (v - st["exp_avg_sq"]).abs().max().item() <= 1e-14
    assert (v[3::7] == 0).all() and (v > 0).sum().item() == 10007 - len(v[3::7])     # the planted zeros, and only they


def test_row_counts_and_workspace_sizes():
    """sk_train_loss_num_blocks and sk_train_loss_workspace_floats are host functions: the rows the table claims (4096
    voxels each, at most 4096 rows), 11 sums per row plus 6 coefficients per sample, and the trips of the other loops."""
    from skoots_amd import _ffi
    rows = [int(_ffi.lib.sk_train_loss_num_blocks(K.voxels(c))) for c, _ in K.TABLE]
    assert rows == [r for _, r in K.TABLE] == [1, 1, 1, 1, 2, 268, 524]
    assert int(_ffi.lib.sk_train_loss_num_blocks(K.CAP_VOXELS)) == 4096 and K.CAP_VOXELS > 4096 * 4096
    assert int(_ffi.lib.sk_train_loss_num_blocks(4096 * 4096)) == 4096 and int(_ffi.lib.sk_train_loss_num_blocks(4097)) == 2
    for (c, r) in K.TABLE:
        assert int(_ffi.lib.sk_train_loss_workspace_floats(c.B, K.voxels(c))) == c.B * r * 11 + c.B * 6
    assert int(_ffi.lib.sk_train_loss_workspace_floats(1, K.CAP_VOXELS)) == 4096 * 11 + 6
    assert max(r for _, r in K.TABLE[:5]) <= 256 < 268                # the finalize loop's second trip starts at 67x129x127
    grid_cap = 4096 * 512                                             # stream_grid(n, 256, 2): loss_bwd, embed_prob, adamw
    assert K.voxels(K.TABLE[5][0]) <= grid_cap < K.voxels(K.TABLE[6][0])
    assert max(K.EMBED_PROB_SIZES) > grid_cap and sorted(K.ADAMW_SIZES)[-2] <= grid_cap < max(K.ADAMW_SIZES)
    assert K.voxels(K.TABLE[5][0]) * K.TABLE[5][0].B > 4096 * 256     # stream_grid(n B, 256): the cldice kernels' second trip
    shapes = [c.shape for c, _ in K.TABLE]
    assert len(set(shapes[2])) == 3 and [K.voxels(c) for c, _ in K.TABLE[:5]] == [1, 105, 1001, 4096, 4352]


@pytest.mark.parametrize("name", K.NAMES)
def test_cases_are_well_conditioned_and_have_their_edges(name):
    case = K.BY_NAME[name]
    d, ref = K.inputs(case), K.loss64(case)
    d32 = K.loss_d32(case)
    print(f"{name}: d32 = {d32:.2e}, losses {ref['losses'].tolist()}, mean pe {ref['pe'].mean().item():.3f}")
    assert d32 <= K.LOSS_D32_MAX
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in d.values())    # handed to the library by pointer
    assert torch.isfinite(ref["losses"]).all() and torch.isfinite(ref["grad"]).all()
    if K.voxels(case) >= 1001 and case.kind == "plain":
        assert 0.15 < ref["pe"].mean().item() < 0.45 and ref["pe"].max().item() > 0.99 and ref["pe"].min().item() < 1e-3
    fg = (d["masks"] > 0).reshape(case.B, -1).sum(dim=1)
    fs = (d["skele"] > 0).reshape(case.B, -1).sum(dim=1)
    g = ref["grad"]
    if case.kind == "edges":
        assert fg[1] == 0 and fs[1] > 0 and fg[2] > 0 and fs[2] == 0 and fg[0] > 0 and fs[0] > 0
        assert (d["masks"][0] == -1).sum() == 24 and (d["masks"][0] == 0.5).sum() == 24
        assert (d["skele"][0] == -1).sum() == 12 and (d["skele"][0] == 0.5).sum() == 12
        # an empty sample has a constant term: channels 0..2 and 4 of sample 1, channel 3 of sample 2 are identically 0
        assert (g[1][..., [0, 1, 2, 4]] == 0).all() and (g[1][..., 3] != 0).any()
        assert (g[2][..., 3] == 0).all() and (g[2][..., [0, 1, 2, 4]] != 0).any()
        for b, x, y, z, c, v in K.PLANTED:
            assert d["logits"][b, x, y, z, c] == v
            if (b, x, y, z, c, v) in K.PLANTED_ZERO:
                assert g[b, x, y, z, c] == 0
            else:       # sigmoid(-40) (1 - sigmoid(-40)) = 4.2e-18: representable, so the derivative is tiny, not 0
                assert 0 < abs(g[b, x, y, z, c].item()) < 1e-17
    if case.kind == "allfg":
        assert fg[0] == K.voxels(case) == fs[0]
    if case.kind == "one":
        assert fg[0] == 1 and fs[0] == 0 and g[0, 0, 0, 0, 3] == 0 and g[0, 0, 0, 0, 4] != 0
    if name == "7x11x13-w010":
        assert (g[..., [0, 1, 2, 3]] == 0).all() and (g[..., 4] != 0).any()


def _shows(case, mut):
    """by what factor a mutated reference leaves the GPU test's bounds on a case: the largest of the four losses' distance
    over loss_bound, a gradient channel's over GRAD_REL of its maximum (inf for a channel that must be exactly 0), and the
    three term fields' over the probability bound"""
    ref, bad = K.loss64(case), K.loss64(case, mut)
    f_loss = float((bad["losses"] - ref["losses"]).abs().max()) / K.loss_bound(case)
    f_grad = K.grad_violations(bad["grad"], ref["grad"])[1] / K.GRAD_REL
    f_prob = max(K.prob_violation(bad[k], ref[k]) for k in ("pe", "ps", "pp"))
    return {"loss": f_loss, "grad": f_grad, "prob": f_prob}


@pytest.mark.parametrize("mut", K.MUTATIONS)
def test_every_loss_mutation_shows(mut):
    """Each deliberate error must leave a bound of the GPU test by more than FACTOR on at least one small case -- in the
    quantity written next to it, so that the table is known to see the error where it was built to."""
    where = {
        "sigma_xy": ("7x11x13", "loss"), "scale_xy": ("7x11x13", "loss"), "decode_xy": ("7x11x13", "loss"),
        # In an all-foreground sample TP + FN = n, so alpha 1e-10 is at most 1e-10 of the denominator: no fp32 loss can see
        # it there (asserted below).  The 1e-10 decides a value only in the empty-sample constant 1 - eps / (alpha 1e-10 +
        # eps) with eps = 1e-8: the probability term of the edges case's sample 1.
        "no_1e10": ("7x11x13-edges", "loss"), "no_eps": ("3x5x7", "loss"), "weight_not_div_B": ("7x11x13", "grad"),
        "prob_skel": ("7x11x13", "loss"), "ne0": ("7x11x13-edges", "loss"), "empty0": ("7x11x13-edges", "loss"),
    }
    name, quantity = where[mut]
    f = _shows(K.BY_NAME[name], mut)
    print(f"{mut} on {name}: {f}")
    assert f[quantity] > FACTOR
    if mut == "weight_not_div_B":
        assert f["loss"] == 0.0                     # the losses cannot see it, only the gradient can
    if mut in ("sigma_xy", "scale_xy", "decode_xy"):
        assert f["grad"] > FACTOR and f["prob"] > FACTOR
    if mut == "no_1e10":
        assert _shows(K.BY_NAME["7x11x13-allfg"], mut)["loss"] < 1e-3
    if mut == "ne0":
        assert f["grad"] > FACTOR
    if mut == "no_eps":
        assert _shows(K.BY_NAME["7x11x13-edges"], mut)["loss"] > FACTOR


def test_symmetric_parameters_would_hide_the_exchanges():
    """What the table is for: with the reference's defaults (sigma x = y, scale x = y) the two exchanges change nothing."""
    case = K.BY_NAME["7x11x13-defaults"]
    for mut in ("sigma_xy", "scale_xy"):
        assert max(_shows(case, mut).values()) == 0.0


@pytest.mark.parametrize("mut", K.ADAMW_MUTATIONS)
def test_every_adamw_mutation_shows(mut):
    """weight decay and eps show with the strong parameters at every step; the bias correction at step 1000 only with the
    defaults' beta2 = 0.999 (0.95^1000 vanishes), which is why the defaults stay a parameter set."""
    params, steps = {"no_decay": ("strong", (0, 1, 2, 3)), "eps_in_sqrt": ("strong", (0, 1, 2, 3)),
                     "no_bias_correction_1000": ("defaults", (3,))}[mut]
    n = 10007
    ref, bad, bounds = K.adamw_run(n, params), K.adamw_run(n, params, torch.float64, mut), K.adamw_bounds(n, params)
    for s in steps:
        factor = ((bad[s][0] - ref[s][0]).abs() / bounds[s][0][1]).max().item()
        print(f"{mut}, {params}, step {K.ADAMW_STEPS[s]}: p leaves its bound by {factor:.3g}")
        assert factor > FACTOR
    if mut == "no_bias_correction_1000":
        s_ref, s_bad = K.adamw_run(n, "strong"), K.adamw_run(n, "strong", torch.float64, mut)
        assert ((s_bad[3][0] - s_ref[3][0]).abs() / K.adamw_bounds(n, "strong")[3][0][1]).max().item() < 1


@pytest.mark.parametrize("params", sorted(K.ADAMW_PARAMS))
def test_adamw_cases_have_their_edges(params):
    lr, _, _, eps, wd = (np.float32(v) for v in K.ADAMW_PARAMS[params])
    assert (np.float32(1) - lr * wd != np.float32(1)) == (params == "strong")       # the decay the old test could not see
    for n in K.ADAMW_SIZES:
        p0, grads = K.adamw_inputs(n)
        zeros = (grads == 0).all(dim=0)
        assert zeros.sum().item() == len(range(3, n, 7)) and (grads[:, ~zeros] != 0).all()
        for (p, m, v), (d32s) in zip(K.adamw_run(n, params), K.adamw_bounds(n, params)):
            assert (v[zeros] == 0).all() and (m[zeros] == 0).all() and torch.isfinite(p).all()
            # p reaches 5.3 (fp32 spacing 4.8e-7) and carries a rounding per step: measured up to 1.1e-6 (p), 6.7e-8 (m),
            # 1.2e-7 (v).  Beyond 2e-6 the fp32 evaluation itself would be off, and 4 d32 no bound
            assert all(d <= 2e-6 for d, _ in d32s)
    g = K.adamw_inputs(2097665)[1].abs()
    assert g[g > 0].min().item() < 1e-9 and g.max().item() > 1.0                      # eight decades of gradient
