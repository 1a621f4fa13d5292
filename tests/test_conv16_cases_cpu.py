"""What makes the assertions of tests/test_hip_conv16_exact.py mean something, checked from the references of
tests/conv16_cases.py and the library's host-only route queries alone (CPU).

The routes: the GPU test claims to run every instantiation sk_conv3d and sk_conv3d_split can launch; that holds only if the
table's cases reach them, which `route` -- conv3d_route of skoots_amd/csrc/conv3d.hip itself, through sk_conv3d_route -- decides
here: every name, threshold and edge asserted below pins the library, and the names sk_conv3d_route_name lists must be the
ones written out in the table.  The plan's numbers are held against conv16_cases.make_plan, an independent restatement.  Integer and split_exact operands: the
GPU test demands bit equality with float64, a fair demand only while every partial accumulation of the kernel, in whatever
order it runs, is exact in fp32 -- the conv's own sums, the 16-bit store and the GroupNorm sums.  Realistic operands: the GPU
test holds the fp16 kernels' GroupNorm totals to d16 / 10 of the definition each implements; that separates "sums of the stored
16-bit values" from "sums of the fp32 accumulators" only if fp32 summation error sits far below d16.
"""
import pytest
import torch

from tests import conv16_cases as K

LIMIT = 2.0 ** 24
IDS = [K.case_id(c) for c in K.ALL]
PRECISIONS = ("fp16", "split")


def test_routes_cover_every_reachable_instantiation():
    """Over the table, the library's route is exactly the 19 fp16 and 8 split instantiations that sk_conv3d and
    sk_conv3d_split can launch in the release build -- written out in conv16_cases.REACHABLE and again here for the ones the
    suite never reached before -- and for every case the name written next to it.  REACHABLE, together with the literal
    lists of the entry points that have no cases here (sk_conv3d_mix8, sk_conv3d_down_act*), is what sk_conv3d_route_name
    lists per precision: a kernel added to the library's tables without a case here fails this test."""
    for prec in PRECISIONS:
        assert {K.route(c, prec) for c in K.ALL} == K.REACHABLE[prec]
        for c in K.ALL:
            assert K.route(c, prec) == K.named(c, prec), (K.case_id(c), prec)
    assert len(K.REACHABLE["fp16"]) == 19 and len(K.REACHABLE["split"]) == 8
    assert K.DOWN_ACT["fp16"] <= K.REACHABLE["fp16"]               # sk_conv3d_down_act runs sk_conv3d's ksize-2 kernels
    for twin in (False, True):
        for prec, want in (("fp16", K.REACHABLE["fp16"]), ("split", K.REACHABLE["split"] | K.DOWN_ACT["split"]),
                           ("mix8", K.MIX8 | K.DOWN_ACT["mix8"])):
            names = K.library_names(prec, twin)
            assert len(names) == len(set(names)) and set(names) == want, (prec, twin, set(names) ^ want)
    assert len(K.MIX8) == 6 and all(len(v) == 2 for v in K.DOWN_ACT.values())
    assert {"m16<3>", "m16<4,3,0>", "gather<32,2>", "gather<64,2>", "gather<128,2>", "conv3<128,2>"} <= K.REACHABLE["fp16"]
    assert {"m16<3,split>", "conv3<64,3,split>"} <= K.REACHABLE["split"]
    assert [K.route(c, "fp16") for c in K.BOX_CASES] == ["px", "m16<4,3,2>", "m16<4,3,1>", "m16<4,3,0>", "m16<3>"]
    assert all(min(c[1]) >= 3 for c in K.BOX_CASES)                 # a box strictly inside the tile exists


def _sweep():
    """the table, and shapes around every threshold of the plan and the dispatch: z 1 .. 129 for the 3x3x3 layer kinds, every
    (cin, cout) pair of ksize 1 and 2"""
    out = list(K.ALL)
    for z in range(1, 130):
        for srcdef, cout in ((K.S32, 32), (K.S64, 32), (K.S64, 64), (K.S128, 128), ([(32, 0), (32, 1)], 32), (K.S32, 64)):
            out.append((1, (8, 8, z if len(srcdef) == 1 else 2 * ((z + 1) // 2)), srcdef, cout, 3))
    for k in (1, 2):
        for c in (32, 64, 128):
            for cout in (32, 64, 128):
                out += [(2, osp, [(c, 0)], cout, k) for osp in ((2, 2, 2), (5, 9, 7), (1, 3, 5))]
    return out


def test_library_plan_equals_the_mirror():
    """Over the table and the sweep, for both precisions and in the bf16 twin: the plan integers sk_conv3d_route reports are
    those of conv16_cases.make_plan, its row count is num_blocks(case) and what sk_conv3d_num_blocks returns (the GPU test
    asserts the same where it runs), the grid is B x rows, and the twin routes every case as the fp16 build does."""
    from skoots_amd import _ffi
    for case in _sweep():
        B, (ox, oy, oz), _, cout, k = case
        for prec in PRECISIONS:
            r = K.library_route(case, prec)
            assert r.num_blocks == K.num_blocks(case) and r.grid == B * r.num_blocks, (K.case_id(case), prec)
            p = K.make_plan(ox, oy, oz, cout) if k == 3 else dict(mode=0, TZ=0, nposp=0, npatch=0, xs=0, lds=0, XC=0, nxc=0)
            assert (r.mode, r.tz, r.nposp, r.npatch, r.xs, r.plan_lds, r.xc, r.nxc) == \
                   tuple(p[key] for key in ("mode", "TZ", "nposp", "npatch", "xs", "lds", "XC", "nxc")), (K.case_id(case), prec)
            assert r.lds >= r.plan_lds or r.name in (b"px", b"pxm")
            t = K.library_route(case, prec, twin=True)
            assert bytes(t) == bytes(r), (K.case_id(case), prec)
        for twin in ("", "_bf16"):
            assert getattr(_ffi.lib, "sk_conv3d_num_blocks" + twin)(B, ox, oy, oz, cout, k) == K.num_blocks(case), K.case_id(case)


def test_library_refuses_what_the_launch_refuses():
    """sk_conv3d_route answers SK_ERR_ARG with the launch's message"""
    for case, prec, msg in (((1, (4, 4, 4), [(48, 0)], 32, 3), "fp16", "multiple of 32 channels"),
                            ((1, (4, 4, 4), K.S32, 48, 3), "fp16", "cout must be 32, 64 or 128"),
                            ((1, (4, 4, 4), [(32, 1)], 32, 3), "fp16", "only the second source may be upsampled"),
                            ((1, (4, 4, 5), [(32, 0), (32, 1)], 32, 3), "split", "even output extents"),
                            ((1, (4, 4, 4), [(128, 0), (128, 0)], 128, 3), "fp16", None),
                            ((1, (4, 4, 4), [(160, 0), (128, 0)], 128, 3), "split", "too many input channels (288)"),
                            ((1, (4, 4, 4), [(32, 0), (32, 0)], 32, 1), "fp16", "ksize 1 takes one plain source"),
                            ((1, (4, 4, 4), [(24, 0)], 32, 1), "fp16", "multiple of 16"),
                            ((1, (4, 4, 4), [(16, 0)], 32, 1), "fp16", "needs 32 <= cin <= 128 (got 16)"),
                            ((1, (4, 4, 4), K.S32, 32, 4), "fp16", "ksize must be 1, 2 or 3")):
        if msg is None:
            assert K.route(case, prec) == "conv3<128,2>"
            continue
        with pytest.raises(ValueError, match=msg.replace("(", r"\(").replace(")", r"\)")):
            K.library_route(case, prec)


def test_route_thresholds_of_cout_32():
    """The z thresholds of the COUT-32 dispatch in linear mode, 6 (nposp + 4) 64 bytes of ring with nposp = ceil16(130 + 2 z):
    <= 15 and 21 .. 23 two tap rows in LDS, 16 .. 20 px for one plain 32-channel source, 24 .. 31 one row, 32 .. 39 none, 40 the
    five-plane ring (in split and with two chunks as well); z > 40 the 8 x 16 rectangles with one row."""
    want = {}
    want.update({z: "m16<4,3,2>" for z in list(range(1, 16)) + [21, 22, 23]})
    want.update({z: "px" for z in range(16, 21)})
    want.update({z: "m16<4,3,1>" for z in list(range(24, 32)) + [41, 48, 70, 128]})
    want.update({z: "m16<4,3,0>" for z in range(32, 40)})
    want[40] = "m16<3>"
    for z, name in want.items():
        assert K.route((1, (8, 8, z), K.S32, 32, 3), "fp16") == name, z
        assert K.route((1, (8, 8, z), K.S32, 32, 3), "split") == ("m16<3,split>" if z == 40 else "m16<4,split>"), z
        two = K.route((1, (8, 8, z), K.S64, 32, 3), "fp16")
        assert two == ("m16<3>" if z == 40 else "m16<4>"), z
    for z in range(1, 130):                                        # COUT 64: the six-plane ring up to z = 23
        assert K.route((1, (8, 8, z), K.S64, 64, 3), "fp16") == ("conv3<64,4>" if z <= 23 else "conv3<64,3>"), z
        assert K.route((1, (8, 8, z), K.S128, 128, 3), "split") == "conv3<128,2,split>", z


def _ragged(case):
    """the last patch (ksize 3) or block (ksize 1 / 2) of a case is ragged: 'linear' | 'rect' | 'block' | None"""
    _, (ox, oy, oz), _, cout, k = case
    if k != 3:
        return "block" if ox * oy * oz % (128 * (1 if cout == 128 else 2)) else None
    p = K.make_plan(ox, oy, oz, cout)
    if p["mode"] == 0:
        return "linear" if oy * oz % 128 else None
    return "rect" if oy % p["TY"] and oz % p["TZ"] else None


def test_case_table_holds_the_edges_it_names():
    """Per kernel family (px, m16, conv3, down2, gather, pointwise in fp16; m16, conv3, gather in split), stated from the shapes: batch 2;
    a ragged last patch (linear and, for m16 and conv3, rectangle mode) or block; ox = 1; z = 5 where the family takes it; for
    the 3x3x3 families an x extent that is no multiple of XS and two or more x-chunks with a ragged last one.  Two sources
    with an upsampled second one for cout 32, 64 and 128; the 128 + 128 concat with 8 chunks (24 = kMaxChunks in split); ksize
    2 on both LDS-staged pairs and on one pair of the gather kernel; ksize 1 with cin 32 (depth 2) and with cin 64 and 128
    (deep, but for the two channel reducers 64 -> 32 and 128 -> 64, which are the pointwise family's) for cout 32, 64 and 128.
    Every case stays under 10^4 output voxels."""
    for prec in PRECISIONS:
        fams = {}
        for c in K.ALL:
            fams.setdefault(K.family(K.route(c, prec)), []).append(c)
        assert set(fams) == ({"px", "m16", "conv3", "down2", "gather", "pointwise"} if prec == "fp16" else {"m16", "conv3", "gather"})
        for fam, cs in fams.items():
            assert any(c[0] == 2 for c in cs), (prec, fam, "batch 2")
            assert any(c[1][0] == 1 for c in cs), (prec, fam, "ox = 1")
            rag = {_ragged(c) for c in cs}
            if fam in ("down2", "gather", "pointwise"):
                assert "block" in rag, (prec, fam)
                assert any(K.num_blocks(c) >= 2 for c in cs), (prec, fam, "more than one block")
                assert any(c[1][2] == 5 for c in cs), (prec, fam, "z = 5")
                continue
            assert "linear" in rag, (prec, fam)
            plans = [K.make_plan(*c[1], c[3]) for c in cs]
            assert any(c[1][0] % p["xs"] for c, p in zip(cs, plans)), (prec, fam, "x % XS")
            assert any(p["nxc"] >= 2 and c[1][0] % p["XC"] for c, p in zip(cs, plans)), (prec, fam, "ragged last x-chunk")
            assert any(p["npatch"] >= 2 for p in plans), (prec, fam, "more than one patch")
            if fam != "px":
                assert "rect" in rag, (prec, fam)
                assert any(c[1][2] == 5 for c in cs), (prec, fam, "z = 5")
    # every m16 / conv3 instantiation on its own: a ragged patch, and a ragged last x-chunk wherever x can be cut
    for name in ("m16<4,3,2>", "m16<4,3,1>", "m16<4,3,0>", "m16<3>", "m16<4>", "conv3<64,4>", "conv3<64,3>", "conv3<128,2>"):
        cs = [c for c in K.ALL if K.route(c, "fp16") == name]
        assert any(_ragged(c) for c in cs), name
        if name not in ("m16<4,3,1>", "m16<4>"):
            assert any(K.make_plan(*c[1], c[3])["nxc"] >= 2 and c[1][0] % K.make_plan(*c[1], c[3])["XC"] for c in cs), name
    ups = {c[3] for c in K.ALL if len(c[2]) == 2}
    assert ups == {32, 64, 128}
    for c in K.ALL:
        for i, ((_, up), shp) in enumerate(zip(c[2], K.source_shapes(c))):
            if up:
                assert c[4] == 3 and i == 1 and all(v % 2 == 0 for v in c[1])
                assert shp[2:] == tuple(v // 2 for v in c[1])
    deep = [c for c in K.ALL if K.cin_of(c) * 27 == 6912 and c[4] == 3]
    assert len(deep) == 1 and deep[0][2] == [(128, 0), (128, 1)] and K.cin_of(deep[0]) // 32 == 8
    assert 3 * K.cin_of(deep[0]) // 32 == K.kMaxChunks
    k2 = {(c[2][0][0], c[3]): K.route(c, "fp16") for c in K.ALL if c[4] == 2}
    assert k2[(32, 64)] == "down2<64,32>" and k2[(64, 128)] == "down2<128,64>" and k2[(64, 64)] == "gather<64,deep>"
    k1 = {(c[2][0][0], c[3]) for c in K.ALL if c[4] == 1}
    assert {(32, 32), (32, 64), (32, 128)} <= k1
    for cout in (32, 64, 128):
        assert K.route((1, (2, 2, 2), K.S32, cout, 1), "fp16") == f"gather<{cout},2>"
        assert (64, cout) in k1 and (128, cout) in k1
    k1_deep = {(c, cout): K.route((1, (2, 2, 2), [(c, 0)], cout, 1), "fp16") for c in (64, 128) for cout in (32, 64, 128)}
    assert k1_deep == {(64, 32): "pointwise<32,64>", (128, 32): "gather<32,deep>", (64, 64): "gather<64,deep>",
                       (128, 64): "pointwise<64,128>", (64, 128): "gather<128,deep>", (128, 128): "gather<128,deep>"}
    for name in ("pointwise<32,64>", "pointwise<64,128>"):          # either reducer on its own: every edge of the block families
        cs = [c for c in K.ALL if K.route(c, "fp16") == name]
        assert any(c[0] == 2 for c in cs) and any(c[1][0] == 1 for c in cs) and any(_ragged(c) for c in cs), name
        assert any(K.num_blocks(c) >= 2 for c in cs) and any(c[1][2] == 5 for c in cs), name
    assert all(c[0] * c[1][0] * c[1][1] * c[1][2] < 10 ** 4 for c in K.ALL)


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_integer_operands_stay_exact(case):
    """conv(|x|, |w|) + |b| < 2^24 everywhere: every partial sum of the fp32 accumulation is an exact integer in any order.
    The reference is integer-valued with |y| <= 2048: the fp16 store, and the hi half of a split store with lo = 0, hold it
    exactly.  Per (sample, quad) sum |y| < 2^24 and sum y^2 < 2^24: every block's partial, a subset of the quad's voxels,
    and every order of adding the blocks is exact.  The operands are what the docstring of tests/conv16_cases.py says.
    Worst over the table: conv(|x|, |w|) + |b| 5 801 and |y| 374 (K = 6912), sum |y| 3.05e5 (B2-5x9x70-32-32-k3), sum y^2 1.58e7
    = 0.94 of 2^24 (B1-5x6x72-64-64-k3; 7 planes of it pass 2^24)."""
    srcs, w, b, y, tot = K.integer_expected(case)
    for t in srcs:
        assert t.min() >= -2 and t.max() <= 2 and torch.equal(t, t.round()) and len(t.unique()) == 5
    assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert b.abs().max() <= 4 and torch.equal(b, b.round())
    mag = K.conv64(case, [t.abs() for t in srcs], w.abs(), b.abs())
    assert mag.max().item() < LIMIT
    assert torch.equal(y, y.round()) and y.abs().max().item() <= 2048
    assert torch.equal(y.half().double(), y)
    a = K.gn_totals(y.abs())[..., 0]
    print(f"{K.case_id(case)}: max sum|x||w|+|b| {mag.max().item():.0f}, max |y| {y.abs().max().item():.0f}, "
          f"quad sum|y| {a.max().item():.0f}, quad sum y^2 {tot[..., 1].max().item():.0f}")
    assert a.max().item() < LIMIT and tot[..., 1].max().item() < LIMIT
    assert tot.shape == (case[0], case[3] // 4, 2) and torch.equal(tot.float().double(), tot)


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_split_exact_operands_stay_exact(case):
    """The packer's halves are the planted ones (fp16(w) = s, w - fp16(w) = j 2^-13, both exact in fp16) and so are the
    activation pairs.  In units of 2^-13 the absolute sum of all three term sets plus |b| stays below 2^24: every partial
    accumulation is exact in any order.  |y| < 2^9 and y a multiple of 2^-13: at most 22 significant bits, which the stored
    pair holds -- join_pair(split_pair(y)) == y.  Worst over the table: 1.03e7 units = 0.61 of 2^24 (K = 1728 at full density;
    K = 3456 at density 0.4: 0.49, K = 6912 at 0.2: 0.48), |y| 156."""
    his, los, w, b, y, _ = K.split_exact_expected(case)
    w_hi = w.half().float()
    w_lo = w - w_hi
    assert set(w_hi.unique().tolist()) == {-1.0, 1.0}
    j = w_lo * 2.0 ** 13
    assert torch.equal(j, j.round()) and j.abs().max() == 3 and torch.equal(w_lo.half().float(), w_lo)
    assert torch.equal(w_hi + w_lo, w)
    for hi, lo in zip(his, los):
        assert set(hi.unique().tolist()) == {-1.0, 0.0, 1.0}
        jl = lo * 2.0 ** 13
        assert torch.equal(jl, jl.round()) and jl.abs().max() == 3 and bool((lo[hi == 0] == 0).all())
        assert torch.equal(hi.half().float(), hi) and torch.equal(lo.half().float(), lo)
    ah, al = [t.abs() for t in his], [t.abs() for t in los]
    mag = (K.conv64(case, ah, w_hi.abs(), b.abs()) + K.conv64(case, ah, w_lo.abs()) + K.conv64(case, al, w_hi.abs())) * 2.0 ** 13
    print(f"{K.case_id(case)}: density {K.split_exact_density(case)}, max sum of |terms| {mag.max().item():.3e} units "
          f"({mag.max().item() / LIMIT:.2f} of 2^24), max |y| {y.abs().max().item():.1f}")
    assert mag.max().item() < LIMIT
    u = y * 2.0 ** 13
    assert torch.equal(u, u.round()) and y.abs().max().item() < 2.0 ** 9
    y32 = y.float()
    assert torch.equal(y32.double(), y)
    assert torch.equal(K.pair_rounded(y32), y32)
    assert (y != K.conv64(case, his, w_hi, b)).any()                # the lo terms do reach the result


@pytest.mark.parametrize("case", K.ALL, ids=IDS)
def test_realistic_totals_separate_stored_values_from_accumulators(case):
    """fp16, realistic operands: the float64 totals of the reference rounded to fp16 (what an epilogue sums that reads the
    stored values) and of the unrounded reference (what one sums that reads its accumulators) lie d16 apart -- the largest
    distance over (sample, quad), for the sums and for the sums of squares.  e_sum, the error of a plain fp32 torch.sum of the
    rounded values (and of their squares) against float64, is at least 100 times smaller: the GPU test's bound d16 / 10
    leaves fp32 accumulation a factor of ten and fails the other definition tenfold.
    Measured over the table: sums d16 3.9e-3 .. 3.3e-2, e_sum 4.8e-7 .. 9.8e-5, ratio 286 .. 10 100; sums of squares d16
    8.4e-3 .. 1.6e-1, e_sum 9.3e-6 .. 1.4e-3, ratio 110 .. 1 580 (the sums of squares are the larger numbers: a single fp32
    rounding of a total costs more of d16 there, and the more the more voxels a case has -- 7 x 5 x 40 voxels gave 82)."""
    *_, d16, e_sum = K.realistic_expected(case)
    print(f"{K.case_id(case)}: sums d16 {d16[0].item():.2e} e_sum {e_sum[0].item():.2e} ratio "
          f"{(d16[0] / e_sum[0].clamp_min(1e-300)).item():.3g} | sums of squares d16 {d16[1].item():.2e} e_sum {e_sum[1].item():.2e} "
          f"ratio {(d16[1] / e_sum[1].clamp_min(1e-300)).item():.3g}")
    assert bool((d16 > 0).all()) and bool((d16 >= 100 * e_sum).all())
