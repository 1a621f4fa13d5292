"""Dice and soft-clDice validation matrices and the validate command (csrc/validate.hip) against the
reference fixture G13 (tests/golden/make_validate_golden.py) and a numpy restatement of the per-slice depth rule
and the contingency counts."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------- numpy restatement

def np_label_skeleton(lab, iters):
    """(X, Y, Z) labels -> uint8 flags: own-label cross-erosion depth per (Y, Z) slice, out-of-slice ignored."""
    lab = np.where(lab > 0, lab, 0).astype(np.int64)
    X, Y, Z = lab.shape
    P = np.pad(lab, ((0, 0), (1, 1), (1, 1)), constant_values=-1)
    D = np.zeros(lab.shape, np.int32)
    kept = lab > 0
    for k in range(1, iters + 2):
        K = np.pad(kept, ((0, 0), (1, 1), (1, 1)), constant_values=False)
        ok = kept.copy()
        for dy, dz in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            nl = P[:, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
            nk = K[:, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
            ok &= (nl == -1) | ((nl == lab) & nk)
        kept = ok
        D[kept] = k
    m = np.minimum(D, iters) + 1
    PD = np.pad(D, ((0, 0), (1, 1), (1, 1)))
    flag = lab > 0
    for dy in (-1, 0, 1):
        for dz in (-1, 0, 1):
            wl = P[:, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
            wd = PD[:, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
            flag &= ~((wl == lab) & (wd >= m))
    return flag.astype(np.uint8)


def np_metrics(gt, pred, iters=3):
    """(iou, dice, cldice) from integer counts, in the reference's fp32 operation order."""
    f = np.float32
    ids_a, ids_b = np.unique(gt[gt > 0]), np.unique(pred[pred > 0])
    N, M = len(ids_a), len(ids_b)
    ra = np.where(gt > 0, np.searchsorted(ids_a, gt) + 1, 0)
    rb = np.where(pred > 0, np.searchsorted(ids_b, pred) + 1, 0)
    cell = (ra * (M + 1) + rb).ravel()
    tail = np.zeros(gt.shape, bool)
    tail[1:] = True
    sg, sp = np_label_skeleton(gt, iters).astype(bool), np_label_skeleton(pred, iters).astype(bool)
    t0 = np.bincount(cell, minlength=(N + 1) * (M + 1)).reshape(N + 1, M + 1)
    tp = np.bincount(cell[(tail & sp).ravel()], minlength=(N + 1) * (M + 1)).reshape(N + 1, M + 1)
    tg = np.bincount(cell[(tail & sg).ravel()], minlength=(N + 1) * (M + 1)).reshape(N + 1, M + 1)
    inter = t0[1:, 1:]
    A, B = t0.sum(1)[1:, None], t0.sum(0)[None, 1:]
    touch = inter > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(touch, inter.astype(f) / (A + B - inter).astype(f), f(0))
        dice = np.where(touch, (2 * inter).astype(f) / (A + B).astype(f), f(0))
        tprec = (tp[1:, 1:].astype(f) + f(1)) / (tp.sum(0)[None, 1:].astype(f) + f(1))
        tsens = (tg[1:, 1:].astype(f) + f(1)) / (tg.sum(1)[1:, None].astype(f) + f(1))
        cl = np.where(touch, f(1) - (f(2) * (tprec * tsens)) / (tprec + tsens), f(0))
    return iou.astype(f), dice.astype(f), cl.astype(f)


def blocky_pair(seed, shape, n_ids, block):
    rng = np.random.default_rng(seed)
    cs = [-(-s // b) for s, b in zip(shape, block)]
    coarse = rng.integers(1, n_ids + 1, cs)
    coarse[rng.random(cs) < 0.3] = 0
    gt = coarse.repeat(block[0], 0).repeat(block[1], 1).repeat(block[2], 2)[:shape[0], :shape[1], :shape[2]]
    gt = gt.copy()
    noise = rng.random(shape) < 0.08
    gt[noise] = rng.integers(0, n_ids + 1, shape)[noise]
    pred = np.roll(gt, (0, 2, -1), (0, 1, 2))
    pred = np.where(pred > 0, (pred * 13 + 5) % (n_ids + 40) + 1, 0)
    noise = rng.random(shape) < 0.05
    pred[noise] = rng.integers(0, n_ids + 41, shape)[noise]
    return gt.astype(np.int32), pred.astype(np.int32)


# ----------------------------------------------------------------------------- fixtures of the reference

def test_pair_fixtures_bit_exact(golden):
    from skoots_amd.validate import mask_dice, mask_iou, mask_metrics, mask_soft_cldice
    d = golden("validate_cldice.npz")
    for name in d["pair_names"]:
        gt, pred = _cuda(d[name + "_gt"]), _cuda(d[name + "_pred"])
        want_dice, want_cl = d[name + "_dice"], d[name + "_cldice"]
        assert np.array_equal(mask_dice(gt, pred).cpu().numpy(), want_dice), name
        assert np.array_equal(mask_soft_cldice(gt, pred).cpu().numpy(), want_cl), name
        iou, dice, cl = mask_metrics(gt, pred)
        assert np.array_equal(dice.cpu().numpy(), want_dice), name
        assert np.array_equal(cl.cpu().numpy(), want_cl), name
        assert np.array_equal(iou.cpu().numpy(), mask_iou(gt, pred).cpu().numpy()), name


def test_skeleton_fixtures_bit_exact(golden):
    from skoots_amd.validate import label_soft_skeleton
    d = golden("validate_cldice.npz")
    for name in d["skel_names"]:
        lab = _cuda(d[name + "_labels"])
        for it in (0, 1, 3, 5):
            got = label_soft_skeleton(lab, it).cpu().numpy()
            assert np.array_equal(got, d[f"{name}_it{it}"]), (name, it)
            assert np.array_equal(got[0], np_label_skeleton(d[name + "_labels"][0], it)), (name, it)
    for name in d["pair_names"]:
        for side in ("gt", "pred"):
            got = label_soft_skeleton(_cuda(d[f"{name}_{side}"])).cpu().numpy()
            assert np.array_equal(got, d[f"{name}_{side}_skel3"]), (name, side)


# ----------------------------------------------------------------------------- a volume of several hundred instances

@pytest.fixture(scope="module")
def big_pair():
    return blocky_pair(4242, (48, 320, 300), 700, (2, 11, 13))


def test_large_volume_equals_numpy(big_pair):
    from skoots_amd.validate import label_soft_skeleton, mask_iou, mask_metrics
    gt, pred = big_pair
    g, p = _cuda(gt[None]), _cuda(pred[None])
    assert np.array_equal(label_soft_skeleton(g).cpu().numpy()[0], np_label_skeleton(gt, 3))
    iou, dice, cl = (t.cpu().numpy() for t in mask_metrics(g, p))
    w_iou, w_dice, w_cl = np_metrics(gt, pred)
    assert iou.shape == w_iou.shape and iou.shape[0] > 300 and iou.shape[1] > 300
    assert np.array_equal(dice, w_dice)
    assert np.array_equal(cl, w_cl)
    assert np.array_equal(iou, w_iou)
    assert np.array_equal(iou, mask_iou(g, p).cpu().numpy())
    assert (cl > 0).sum() > 1000


@pytest.mark.parametrize("iters", [0, 1, 5, 12])
def test_other_iters_equal_numpy(iters):
    from skoots_amd.validate import label_soft_skeleton, mask_metrics
    gt, pred = blocky_pair(77 + iters, (5, 90, 150), 60, (1, 17, 19))
    g, p = _cuda(gt[None]), _cuda(pred[None])
    assert np.array_equal(label_soft_skeleton(g, iters).cpu().numpy()[0], np_label_skeleton(gt, iters))
    for got, want in zip(mask_metrics(g, p, iters), np_metrics(gt, pred, iters)):
        assert np.array_equal(got.cpu().numpy(), want)


def test_repeatable(big_pair):
    from skoots_amd.validate import mask_metrics
    g, p = _cuda(big_pair[0][None]), _cuda(big_pair[1][None])
    first = [t.cpu().numpy() for t in mask_metrics(g, p)]
    second = [t.cpu().numpy() for t in mask_metrics(g, p)]
    for a, b in zip(first, second):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- deliberate differences

def test_identical_instance_dice_is_one():
    from skoots_amd.validate import mask_dice, mask_metrics
    gt = torch.zeros((1, 4, 20, 20), dtype=torch.int32, device=DEV)
    gt[0, :, 2:9, 3:12] = 4
    gt[0, 1:, 12:18, 5:15] = 9
    pred = torch.where(gt > 0, gt + 100, gt)
    pred[0, 0, 12:18, 5:15] = 109                     # 9's match grows by one slice
    dice = mask_dice(gt, pred).cpu().numpy()
    assert dice[0, 0] == 1.0 and dice[1, 1] == np.float32(2 * 180) / np.float32(180 + 240)
    iou, dice2, cl = mask_metrics(gt, pred)
    assert iou[0, 0].item() == 1.0 and dice2[0, 0].item() == 1.0 and cl[0, 0].item() == 0.0


def test_empty_volumes_and_layouts():
    from skoots_amd.validate import label_soft_skeleton, mask_dice, mask_metrics, mask_soft_cldice
    z = torch.zeros((1, 3, 9, 9), dtype=torch.int32, device=DEV)
    for t in mask_metrics(z, z):
        assert t.shape == (0, 0)
    one = z.clone()
    one[0, 1, 2:5, 2:5] = 3
    iou, dice, cl = mask_metrics(one, z)
    assert iou.shape == dice.shape == cl.shape == (1, 0)
    assert mask_dice(one.reshape(3, 9, 9), one.reshape(3, 9, 9)).shape == (1, 1)   # counts only: any shape
    for bad in (one[0], one[None], torch.cat([one, one])):
        with pytest.raises(ValueError, match=r"\(1, X, Y, Z\)"):
            mask_soft_cldice(bad, bad)
        with pytest.raises(ValueError, match=r"\(1, X, Y, Z\)"):
            label_soft_skeleton(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mask_soft_cldice(one.cpu(), one.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        label_soft_skeleton(one.cpu())
    with pytest.raises(ValueError, match="iters"):
        mask_metrics(one, one, iters=13)


def test_rows_follow_positive_ids_without_background():
    from skoots_amd.validate import mask_metrics
    from skoots_amd.validate.__main__ import format_reports
    gt = torch.full((1, 3, 10, 10), 5, dtype=torch.int32, device=DEV)
    gt[0, :, 5:] = 8                                  # no background voxel
    pred = gt.clone()
    pred[0, :, :, :3] = 0
    iou, dice, cl = mask_metrics(gt, pred)
    _, text = format_reports("g", "p", iou, dice, cl, [5, 8])
    rows = text.splitlines()[6:]
    assert [r.split(",")[0] for r in rows] == ["5", "8"]
    assert float(rows[0].split(",")[1]) == iou[0].max().item()


# ----------------------------------------------------------------------------- refused calls

def test_refused_calls_leave_outputs_untouched():
    from skoots_amd import _ffi
    L = _ffi.lib
    gt = torch.zeros((1, 2, 8, 8), dtype=torch.int32, device=DEV)
    gt[0, :, 1:4, 1:5] = 1
    pred = gt.clone()
    lut = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    outs = [torch.full((1, 1), -7.0, device=DEV) for _ in range(3)]
    ws_bytes = int(L.sk_mask_metrics_workspace_bytes(1, 1))
    ws = torch.full((ws_bytes,), 0xAB, dtype=torch.uint8, device=DEV)
    st = _ffi.stream_ptr(gt.device)
    P = _ffi.ptr

    def call(X=2, Y=8, Z=8, lut_a=lut, N=1, M=1, iters=3, ws_b=ws_bytes, gt_p=gt):
        return L.sk_mask_metrics(P(gt_p), P(pred), X, Y, Z, P(lut_a), 1, N, P(lut), 1, M, iters,
                                 *(P(o) for o in outs), P(ws), ws_b, st)

    for kw in (dict(X=0), dict(Z=-1), dict(X=1 << 16, Y=1 << 15, Z=1), dict(lut_a=None), dict(gt_p=None),
               dict(N=-1), dict(iters=-1), dict(iters=13), dict(ws_b=ws_bytes - 1),
               dict(N=1 << 16, M=1 << 15)):
        assert call(**kw) == -1, kw
    skel = torch.full((1, 2, 8, 8), 0x5A, dtype=torch.uint8, device=DEV)
    for args in ((2, 8, 8, 13), (0, 8, 8, 3), (2, 8, 8, -1), (1 << 16, 1 << 16, 1, 3)):
        assert L.sk_label_soft_skeleton2d(P(gt), *args, P(skel), st) == -1, args
    assert L.sk_label_soft_skeleton2d(None, 2, 8, 8, 3, P(skel), st) == -1
    torch.cuda.synchronize()
    for o in outs:
        assert o.item() == -7.0
    assert bool((ws == 0xAB).all()) and bool((skel == 0x5A).all())
    assert call() == 0                                # the same buffers, accepted
    torch.cuda.synchronize()
    assert [o.item() for o in outs] == [1.0, 1.0, 0.0]


# ----------------------------------------------------------------------------- the command

def test_command_writes_the_reference_csv(golden, tmp_path, monkeypatch):
    from skoots_amd.lib.eval import _write_mask_tif
    from skoots_amd.validate.__main__ import main
    d = golden("validate_cldice.npz")
    _write_mask_tif(str(tmp_path / "gt.tif"), d["csv_gt_zxy"])
    _write_mask_tif(str(tmp_path / "pred.tif"), d["csv_pred_zxy"])
    monkeypatch.chdir(tmp_path)
    acc_path, iou_path = main(["--ground_truth", "gt.tif", "--predicted", "pred.tif"])
    assert acc_path == "pred_accuracy_stats.csv" and iou_path == "pred_intersection_over_union.csv"
    with open(acc_path) as f:
        assert f.read() == str(d["csv_accuracy"])
    with open(iou_path) as f:
        assert f.read() == str(d["csv_iou"])


def test_command_reads_npy(golden, tmp_path, monkeypatch):
    from skoots_amd.validate.__main__ import main
    d = golden("validate_cldice.npz")
    np.save(tmp_path / "gt.npy", d["csv_gt_zxy"].astype(np.int32))
    np.save(tmp_path / "pred.npy", d["csv_pred_zxy"].astype(np.int32))
    monkeypatch.chdir(tmp_path)
    main(["--ground_truth", "gt.npy", "--predicted", "pred.npy", "--log", "4"])
    with open("pred_intersection_over_union.csv") as f:
        text = f.read()
    assert text.replace(".npy", ".tif") == str(d["csv_iou"])
