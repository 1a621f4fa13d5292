"""The cases, plan mirror, seeded operands and float64 references that tests/test_conv16_cases_cpu.py and
tests/test_hip_conv16_exact.py share (torch on the CPU only): the fp16 and split conv kernels of skoots_amd/csrc/conv3d.hip
behind sk_conv3d, sk_conv3d_split and sk_conv3d_box.

A case is ``(B, out spatial, [(C, up)], cout, ksize)``: the layer's sources are concatenated along the channels, a source
with ``up`` is stored at half the output extent and read through a nearest upsample; ksize 3 has padding 1 and stride 1,
ksize 2 stride 2, ksize 1 stride 1.  CASES holds, next to every case, the instantiation it runs in precision "fp16" and in
precision "split" -- what ``route`` returns for it, which is the library's own answer: conv3d_route of
skoots_amd/csrc/conv3d.hip, the one function the launches ask, through the host-only sk_conv3d_route.  tests/test_conv16_cases_cpu.py
asserts both columns and that together they cover every name sk_conv3d_route_name lists.  ``make_plan`` and ``num_blocks``
stay an independent restatement of the plan's numbers, compared with the library's.  Each case is the smallest shape that
reaches its branch and edge.

Route names:
``px``                conv3_px_kernel (32 -> 32, one plain source, z 16 .. 20)
``m16<4,3,W>``        conv3_m16_kernel<32, 4, 3, false, W>: single chunk, 3 tap rows in registers, W more in LDS
``m16<4>`` ``m16<3>`` conv3_m16_kernel<32, XS>: several chunks, or the five-plane ring of z = 40
``conv3<C,XS>``       conv3_kernel<C, XS>;   ``..,split>``: the SPLIT form of any of the above
``down2<C,CIN>``      down2_act_kernel<C, CIN> without activation (fp16, ksize 2, 32 -> 64 | 64 -> 128)
``gather<C,deep|2>``  gather_gemm_kernel<C, PV, 4 | 2>;   ``gather<C,split>``: gather_gemm_kernel<C, PV, 2, true>
``pointwise<C,CIN>``  pointwise_lds_kernel<C, CIN> (fp16, ksize 1, 64 -> 32 | 128 -> 64: the channel reducers)

Three kinds of operands:

``integer``      activations uniform integers in [-2, 2], weights in {-1, 0, 1}, biases in [-4, 4]; for split the same values
                 go in as pairs with lo = 0.  Every fp16 product is an exact integer and the MFMAs accumulate in fp32, so
                 while sum |x||w| + |b| stays below 2^24 every partial accumulation is an exact integer in ANY order: the
                 kernel must equal the float64 conv bit for bit (|y| <= 2048: the fp16 store is exact too), and so must the
                 GroupNorm totals while sum |y| and sum y^2 per (sample, quad) stay below 2^24.
``split_exact``  split only.  Activation pairs built directly (never through split_pair): hi in {-1, 0, 1}, lo = j 2^-13 with
                 j in [-3, 3], lo = 0 where hi = 0; weights w = s + j 2^-13, s = +-1 (never 0) and j in [-3, 3] -- a j that points
                 towards zero by more than one unit is mirrored, fp16's spacing below 1 being 2^-11 --, so the packer's
                 hi = fp16(w) is s and its lo is j 2^-13; integer biases in [-4, 4].  The reference is the arithmetic as DEFINED,
                 conv(x_hi, w_hi) + conv(x_hi, w_lo) + conv(x_lo, w_hi) + b with no lo * lo term: every term is a multiple of
                 2^-13, exact in fp32 while the absolute sum stays below 2^24 units.  The nonzero hi are thinned out for the
                 deep contractions (density 0.4 above K = 1728, 0.2 above K = 3456).
``realistic``    randn activations rounded to what the precision holds, randn / sqrt(cin k^3) weights, 0.1 randn biases.

The GroupNorm partial layout (include/skoots_hip.h): sk_conv3d_num_blocks rows per sample, a row holding per quad of four
consecutive output channels the sum and the sum of squares over the voxels of one workgroup.  Which voxels a workgroup
owns differs from kernel to kernel; what the interface promises, and what these tests hold, are the row count and the
rows' totals.
"""
import functools

import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------------- what the library says
PRECISION_CODE = {"fp16": 0, "split": 1, "mix8": 2}      # SK_CONV_FP16, SK_CONV_SPLIT, SK_CONV_MIX8


def library_route(case, precision, twin=False):
    """sk_conv3d_route (host only: no GPU) for a case as sk_conv3d / sk_conv3d_split would launch it -> the filled
    skoots_amd._ffi.ConvRoute; ValueError with the launch's message for a shape the launch refuses"""
    from skoots_amd import _ffi
    B, (ox, oy, oz), srcdef, cout, k = case
    arr = (_ffi.ConvSrc * len(srcdef))()
    for a, (c, up) in zip(arr, srcdef):
        a.data, a.affine, a.c, a.upsample = None, None, c, up
    r = _ffi.ConvRoute()
    fn = getattr(_ffi.lib, "sk_conv3d_route" + ("_bf16" if twin else ""))
    _ffi.check(fn(0, PRECISION_CODE[precision], arr, len(srcdef), B, ox, oy, oz, cout, k, r))
    return r


def route(case, precision):
    """The instantiation sk_conv3d (precision "fp16") or sk_conv3d_split ("split") launches for a case: conv3d_route of
    skoots_amd/csrc/conv3d.hip, asked through sk_conv3d_route"""
    assert precision in ("fp16", "split")
    return library_route(case, precision).name.decode()


def library_names(precision, twin=False):
    """sk_conv3d_route_name until NULL: every kernel a launch of the precision can reach"""
    from skoots_amd import _ffi
    fn = getattr(_ffi.lib, "sk_conv3d_route_name" + ("_bf16" if twin else ""))
    names = []
    while fn(PRECISION_CODE[precision], len(names)) is not None:
        names.append(fn(PRECISION_CODE[precision], len(names)).decode())
    return names


# ---------------------------------------------------------------------------------------------- the plan mirror
# An independent restatement of the numbers conv3d_route hands a launch; tests compare the library's with these.
kPosBytes = 64            # skoots_amd/csrc/conv3_device.h
kPatch = 128              # skoots_amd/csrc/conv3_device.h
kPadBytes = 32 * 64       # skoots_amd/csrc/conv3_device.h (32 * kPadStride)
kZeroPos = 4              # skoots_amd/csrc/common.h (SK_ZERO_WINDOW, the default build)
kMaxDma = 4               # skoots_amd/csrc/conv3d.hip
kMaxChunks = 24           # skoots_amd/csrc/conv3d.hip
kLdsTwoPerCU = 80 * 1024  # make_plan, conv3d_route: two workgroups per CU need <= 80 KiB each
kPlanBatch = 8            # make_plan
kTarget = 256 * 2 * 8     # make_plan (`target`)


def make_plan(ox, oy, oz, cout):
    """make_plan (skoots_amd/csrc/conv3d.hip) -> dict(mode, TY, TZ, nposp, npatch, xs, lds, XC, nxc), or None where it
    refuses the plane geometry"""
    xs = 2 if cout == 128 else 4                                   # conv3_xs
    if oz <= 40:
        mode, TZ, TY = 0, oz, None
        npatch = (oy * oz + kPatch - 1) // kPatch
        nposp = (kPatch + 2 * oz + 2 + 15) // 16 * 16
    else:
        mode, TZ = 1, (16 if cout == 32 else 32)
        TY = kPatch // TZ
        nzc = (oz + TZ - 1) // TZ
        npatch = ((oy + TY - 1) // TY) * nzc
        nposp = ((TY + 2) * (TZ + 2) + 15) // 16 * 16
    if nposp > 64 * kMaxDma:
        return None
    pads = 0 if cout == 32 else 4 * kPadBytes
    lds = (xs + 2) * (nposp + kZeroPos) * kPosBytes + pads
    if xs == 4 and lds > kLdsTwoPerCU:
        xs = 3
        lds = (xs + 2) * (nposp + kZeroPos) * kPosBytes + pads
    nxc = (kTarget + npatch * kPlanBatch - 1) // (npatch * kPlanBatch)
    if cout == 32 and mode == 0:
        nxc = 2 if nxc >= 4 else (nxc + 1) // 2
    nxc = max(1, min(nxc, (ox + 2 * xs - 1) // (2 * xs)))
    XC = (ox + nxc - 1) // nxc
    XC = (XC + xs - 1) // xs * xs
    return dict(mode=mode, TY=TY, TZ=TZ, nposp=nposp, npatch=npatch, xs=xs, lds=lds, XC=XC, nxc=(ox + XC - 1) // XC)


def num_blocks(case):
    """sk_conv3d_num_blocks: rows of gn_partial per sample"""
    _, (ox, oy, oz), _, cout, k = case
    if k == 3:
        p = make_plan(ox, oy, oz, cout)
        return p["npatch"] * p["nxc"]
    per = 128 * (1 if cout == 128 else 2)
    return (ox * oy * oz + per - 1) // per


# ---------------------------------------------------------------------------------------------- the case table
S32, S64, S128 = [(32, 0)], [(64, 0)], [(128, 0)]
CASES = [
    # ((B, out spatial, [(C, up)], cout, ksize), route in fp16, route in split)
    # ---- px: 176-position planes, z 16 .. 20
    ((2, (5, 7, 20), S32, 32, 3), "px", "m16<4,split>"),             # batch 2, 140 voxels a plane: ragged second patch, odd x
    ((1, (9, 7, 18), S32, 32, 3), "px", "m16<4,split>"),             # two x-chunks of 8 + 1 planes
    ((1, (1, 7, 16), S32, 32, 3), "px", "m16<4,split>"),             # ox = 1, one ragged patch
    # ---- m16, single chunk
    ((2, (5, 9, 5), S32, 32, 3), "m16<4,3,2>", "m16<4,split>"),      # z = 5, batch 2, 45 voxels a plane, x % 4 != 0
    ((1, (9, 7, 22), S32, 32, 3), "m16<4,3,2>", "m16<4,split>"),     # z 22: px's plane size, too few padding positions; 8 + 1 planes
    ((1, (1, 13, 10), S32, 32, 3), "m16<4,3,2>", "m16<4,split>"),    # ox = 1, 130 voxels: a second patch of two voxels
    ((1, (5, 6, 24), S32, 32, 3), "m16<4,3,1>", "m16<4,split>"),     # linear, z 24 .. 31
    ((2, (5, 9, 70), S32, 32, 3), "m16<4,3,1>", "m16<4,split>"),     # 8 x 16 rectangles: y % 8 != 0, z % 16 != 0, batch 2
    ((1, (5, 5, 33), S32, 32, 3), "m16<4,3,0>", "m16<4,split>"),     # z 32 .. 39: no tap rows in LDS
    ((1, (9, 4, 39), S32, 32, 3), "m16<4,3,0>", "m16<4,split>"),     # ... 8 + 1 planes
    ((2, (5, 4, 40), S32, 32, 3), "m16<3>", "m16<3,split>"),         # z = 40: the five-plane ring; x % 3 != 0, batch 2
    ((1, (7, 3, 40), S32, 32, 3), "m16<3>", "m16<3,split>"),         # ... x-chunks of 6 + 1 planes, one patch of 120 voxels
    # ---- m16, several chunks
    ((1, (6, 6, 10), [(32, 0), (32, 1)], 32, 3), "m16<4>", "m16<4,split>"),    # concat with an upsampled second source
    ((2, (5, 7, 12), S64, 32, 3), "m16<4>", "m16<4,split>"),                   # two chunks of one source
    ((1, (4, 10, 44), [(32, 0), (32, 1)], 32, 3), "m16<4>", "m16<4,split>"),   # ... on rectangles: y % 8, z % 16 != 0
    ((1, (4, 4, 40), [(32, 0), (32, 1)], 32, 3), "m16<3>", "m16<3,split>"),    # ... on the five-plane ring
    # ---- conv3
    ((2, (5, 7, 10), S64, 64, 3), "conv3<64,4>", "conv3<64,4,split>"),         # batch 2, ragged patch, x % 4 != 0
    ((1, (13, 5, 10), S64, 64, 3), "conv3<64,4>", "conv3<64,4,split>"),        # x-chunks of 8 + 5 planes
    ((1, (1, 13, 10), S32, 64, 3), "conv3<64,4>", "conv3<64,4,split>"),        # ox = 1, single chunk
    ((1, (6, 8, 10), [(64, 0), (64, 1)], 64, 3), "conv3<64,4>", "conv3<64,4,split>"),   # concat + upsample
    ((1, (7, 5, 24), S64, 64, 3), "conv3<64,3>", "conv3<64,3,split>"),         # linear, z >= 24: the five-plane ring; 6 + 1 planes
    ((1, (5, 6, 72), S64, 64, 3), "conv3<64,3>", "conv3<64,3,split>"),         # 4 x 32 rectangles: y % 4, z % 32, x % 3 != 0
    ((1, (7, 19, 5), S128, 128, 3), "conv3<128,2>", "conv3<128,2,split>"),     # z = 5, x-chunks of 4 + 3 planes
    ((2, (1, 9, 16), S128, 128, 3), "conv3<128,2>", "conv3<128,2,split>"),     # ox = 1, batch 2, ragged second patch
    ((1, (3, 5, 44), S128, 128, 3), "conv3<128,2>", "conv3<128,2,split>"),     # rectangles, x % 2 != 0
    ((1, (4, 6, 4), [(128, 0), (128, 1)], 128, 3), "conv3<128,2>", "conv3<128,2,split>"),   # K = 6912: 8 chunks, 24 in split
    # ---- ksize 2: the LDS-staged pairs (fp16) and one pair of the gather kernel
    ((2, (3, 5, 4), S32, 64, 2), "down2<64,32>", "gather<64,split>"),          # batch 2, 60 of a block's 256 voxels
    ((1, (5, 9, 7), S32, 64, 2), "down2<64,32>", "gather<64,split>"),          # 315 voxels: two blocks, ragged
    ((1, (5, 9, 5), S64, 128, 2), "down2<128,64>", "gather<128,split>"),       # 225 voxels: two blocks of 128, ragged
    ((2, (1, 3, 5), S64, 128, 2), "down2<128,64>", "gather<128,split>"),       # ox = 1, batch 2
    ((2, (3, 5, 7), S64, 64, 2), "gather<64,deep>", "gather<64,split>"),       # a pair launch_down2 does not take
    # ---- ksize 1
    ((2, (5, 9, 7), S32, 32, 1), "gather<32,2>", "gather<32,split>"),          # cin 32: two K steps, depth 2; two blocks, ragged
    ((1, (1, 9, 10), S32, 64, 1), "gather<64,2>", "gather<64,split>"),         # ox = 1
    ((1, (5, 9, 5), S32, 128, 1), "gather<128,2>", "gather<128,split>"),
    ((1, (12, 5, 5), S64, 32, 1), "pointwise<32,64>", "gather<32,split>"),     # 300 voxels: two blocks, ragged; z = 5
    ((2, (1, 9, 5), S64, 32, 1), "pointwise<32,64>", "gather<32,split>"),      # ox = 1, batch 2
    ((2, (3, 7, 10), S128, 32, 1), "gather<32,deep>", "gather<32,split>"),
    ((1, (5, 7, 9), S64, 64, 1), "gather<64,deep>", "gather<64,split>"),
    ((1, (9, 10, 5), S128, 64, 1), "pointwise<64,128>", "gather<64,split>"),   # 450 voxels: two blocks, ragged; z = 5
    ((2, (1, 9, 5), S128, 64, 1), "pointwise<64,128>", "gather<64,split>"),    # ox = 1, batch 2
    ((1, (5, 3, 9), S64, 128, 1), "gather<128,deep>", "gather<128,split>"),    # 135 voxels: a second block of seven
    ((2, (1, 5, 9), S128, 128, 1), "gather<128,deep>", "gather<128,split>"),   # ox = 1, batch 2
]
ALL = [c for c, _, _ in CASES]


def named(case, precision):
    """the route written next to a case in CASES"""
    return CASES[ALL.index(case)][1 if precision == "fp16" else 2]


# every instantiation sk_conv3d ("fp16") and sk_conv3d_split ("split") can launch in the release build: literal, and held
# equal to what sk_conv3d_route_name lists (tests/test_conv16_cases_cpu.py), so that a kernel added to the library's tables
# without a case here fails on the CPU
REACHABLE = {
    "fp16": {"px", "m16<4,3,2>", "m16<4,3,1>", "m16<4,3,0>", "m16<4>", "m16<3>", "conv3<64,4>", "conv3<64,3>", "conv3<128,2>",
             "down2<64,32>", "down2<128,64>", "gather<32,deep>", "gather<32,2>", "gather<64,deep>", "gather<64,2>",
             "gather<128,deep>", "gather<128,2>", "pointwise<32,64>", "pointwise<64,128>"},
    "split": {"m16<4,split>", "m16<3,split>", "conv3<64,4,split>", "conv3<64,3,split>", "conv3<128,2,split>",
              "gather<32,split>", "gather<64,split>", "gather<128,split>"},
}
# the names without cases in this table (tests/test_hip_unet.py runs them against torch): what sk_conv3d_mix8 launches, and
# the LDS-staged stride-2 pairs of sk_conv3d_down_act (fp16: the kernels of sk_conv3d's ksize 2), _split and _mix8
MIX8 = {"pxm", "m16<4,mix8>", "m16<3,mix8>", "conv3<64,4,mix8>", "conv3<64,3,mix8>", "conv3<128,2,mix8>"}
DOWN_ACT = {"fp16": {"down2<64,32>", "down2<128,64>"}, "split": {"down2<64,32,split>", "down2<128,64,split>"},
            "mix8": {"down2<64,32,split>", "down2<128,64,split>"}}
# one case per route that honours a store box, each with x >= 3 so that a box fits strictly inside
BOX_CASES = [ALL[0], ALL[3], ALL[6], ALL[8], ALL[10]]


def family(name):
    """px | m16 | conv3 | down2 | gather | pointwise"""
    return name.split("<")[0]


def case_id(case):
    B, osp, srcdef, cout, k = case
    return f"B{B}-{'x'.join(map(str, osp))}-" + "+".join(f"{c}{'u' if up else ''}" for c, up in srcdef) + f"-{cout}-k{k}"


def cin_of(case):
    return sum(c for c, _ in case[2])


def source_shapes(case):
    """[(B, C, xs, ys, zs)]: the stored shape of every source, channels first"""
    B, osp, srcdef, _, k = case
    s = 2 if k == 2 else 1
    return [(B, c) + (tuple(v // 2 for v in osp) if up else tuple(v * s for v in osp)) for c, up in srcdef]


def _seed(case, kind):
    B, osp, srcdef, cout, k = case
    return 1000 * kind + 97 * B + 31 * osp[0] + 17 * osp[1] + 7 * osp[2] + 5 * cout + 3 * k + sum(c + up for c, up in srcdef)


# ---------------------------------------------------------------------------------------------- the operands
def split_pair(x):
    """fp32 (..., C) -> the split layout (..., 2C) fp16 = [hi | lo], hi = fp16(x), lo = fp16(x - hi) (skoots_amd.unet.split_pair)"""
    hi = x.half()
    return torch.cat([hi, (x - hi.float()).half()], dim=-1).contiguous()


def join_pair(x):
    """split layout (..., 2C) fp16 -> fp32 (..., C) = hi + lo (skoots_amd.unet.join_pair)"""
    c = x.shape[-1] // 2
    return x[..., :c].float() + x[..., c:].float()


def pair_rounded(t):
    """t (fp32) rounded to what a split pair holds"""
    return join_pair(split_pair(t.unsqueeze(-1))).squeeze(-1)


def integer_operands(case):
    """(sources, weight, bias) float32, integer-valued: activations in [-2, 2], weights in {-1, 0, 1}, biases in [-4, 4]"""
    _, _, _, cout, k = case
    g = torch.Generator().manual_seed(_seed(case, 1))
    srcs = [torch.randint(-2, 3, shp, generator=g).float() for shp in source_shapes(case)]
    w = torch.randint(-1, 2, (cout, cin_of(case), k, k, k), generator=g).float()
    b = torch.randint(-4, 5, (cout,), generator=g).float()
    return srcs, w, b


def split_exact_density(case):
    """share of nonzero candidates among the activations' hi halves: thinner for the deep contractions"""
    K = cin_of(case) * case[4] ** 3
    return 0.2 if K > 3456 else 0.4 if K > 1728 else 1.0


def split_exact_operands(case):
    """(hi sources, lo sources, weight, bias) float32: hi in {-1, 0, 1} (thinned by split_exact_density), lo = j 2^-13 with
    j in [-3, 3] and 0 where hi = 0; weight = s + j 2^-13 with s = +-1 and j s in [-1, 3] (below 1 fp16's spacing is 2^-11 = 4
    units: s - 2 s 2^-13 would be a tie and s - 3 s 2^-13 round to the neighbour of s); bias integer in [-4, 4]"""
    _, _, _, cout, k = case
    g = torch.Generator().manual_seed(_seed(case, 3))
    dens = split_exact_density(case)
    his, los = [], []
    for shp in source_shapes(case):
        hi = torch.randint(-1, 2, shp, generator=g).float() * (torch.rand(shp, generator=g) < dens).float()
        lo = torch.randint(-3, 4, shp, generator=g).float() * 2.0 ** -13 * (hi != 0).float()
        his.append(hi)
        los.append(lo)
    shp = (cout, cin_of(case), k, k, k)
    s = (torch.randint(0, 2, shp, generator=g) * 2 - 1).float()
    j = torch.randint(-3, 4, shp, generator=g).float()
    j = torch.where(j * s < -1, -j, j)
    w = s + j * 2.0 ** -13
    b = torch.randint(-4, 5, (cout,), generator=g).float()
    return his, los, w, b


def realistic_operands(case, precision="fp16"):
    """(sources, weight, bias) float32: randn rounded to what the precision's activations hold (fp16, or a split pair),
    randn / sqrt(cin k^3), 0.1 randn"""
    _, _, _, cout, k = case
    g = torch.Generator().manual_seed(_seed(case, 2))
    hold = (lambda t: t.half().float()) if precision == "fp16" else pair_rounded
    srcs = [hold(torch.randn(shp, generator=g)) for shp in source_shapes(case)]
    cin = cin_of(case)
    w = torch.randn((cout, cin, k, k, k), generator=g) / (cin * k ** 3) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return srcs, w, b


# ---------------------------------------------------------------------------------------------- the references
def assemble(case, srcs):
    """The conv's input (B, cin, ...) in the sources' dtype: upsampled sources through a nearest upsample, concatenated"""
    xs = [F.interpolate(t, scale_factor=2, mode="nearest") if up else t for t, (_, up) in zip(srcs, case[2])]
    return torch.cat(xs, dim=1)


def conv64(case, srcs, w, b=None):
    """float64 F.conv3d of the assembled sources -> (B, cout, ox, oy, oz)"""
    k = case[4]
    x = assemble(case, [t.double() for t in srcs])
    b = None if b is None else b.double()
    return F.conv3d(x, w.double(), b, padding=1) if k == 3 else F.conv3d(x, w.double(), b, stride=k)


def gn_totals(y):
    """y (B, cout, ox, oy, oz) -> (B, cout / 4, 2) float64: per sample and quad of four consecutive channels, the sum and the
    sum of squares over the sample's voxels"""
    B, cout = y.shape[:2]
    v = y.double().reshape(B, cout // 4, -1)
    return torch.stack([v.sum(dim=-1), (v * v).sum(dim=-1)], dim=-1)


def gn_totals_f32(y):
    """gn_totals by a plain fp32 torch.sum of the fp32 values (and of their fp32 squares), as float64"""
    B, cout = y.shape[:2]
    v = y.float().reshape(B, cout // 4, -1)
    return torch.stack([v.sum(dim=-1), (v * v).sum(dim=-1)], dim=-1).double()


@functools.lru_cache(maxsize=None)
def _integer(idx):
    srcs, w, b = integer_operands(ALL[idx])
    y = conv64(ALL[idx], srcs, w, b)
    return srcs, w, b, y, gn_totals(y)


@functools.lru_cache(maxsize=None)
def _split_exact(idx):
    case = ALL[idx]
    his, los, w, b = split_exact_operands(case)
    w_hi = w.half().float()
    w_lo = w - w_hi
    y = conv64(case, his, w_hi, b) + conv64(case, his, w_lo) + conv64(case, los, w_hi)
    return his, los, w, b, y, gn_totals(y)


@functools.lru_cache(maxsize=None)
def _realistic(idx):
    case = ALL[idx]
    srcs, w, b = realistic_operands(case, "fp16")
    y = conv64(case, srcs, w.half(), b)                             # the operands the kernel multiplies: fp16 weights
    y16 = y.half().double()
    t_acc, t_st = gn_totals(y), gn_totals(y16)
    d16 = (t_acc - t_st).abs().amax(dim=(0, 1))                    # (2,): sums, sums of squares
    e_sum = (gn_totals_f32(y16) - t_st).abs().amax(dim=(0, 1))
    return srcs, w, b, y, t_acc, t_st, d16, e_sum


def integer_expected(case):
    """(sources, weight, bias, float64 conv, float64 totals (B, cout / 4, 2)); computed once, not to be modified"""
    return _integer(ALL.index(case))


def split_exact_expected(case):
    """(hi sources, lo sources, weight, bias, the defined three-term float64 result, its totals); computed once, not to be
    modified"""
    return _split_exact(ALL.index(case))


def realistic_expected(case):
    """fp16: (sources, weight, bias, y = float64 conv of the fp16 activations and fp16-rounded weights, totals of y -- the
    accumulators' definition --, totals of fp16(y) -- the stored values' definition --, d16 (2,) = the largest distance of
    the two over (sample, quad) for the sums and for the sums of squares, e_sum (2,) = the largest error of a plain fp32
    torch.sum of the stored values, and of their squares, against float64); computed once, not to be modified"""
    return _realistic(ALL.index(case))
