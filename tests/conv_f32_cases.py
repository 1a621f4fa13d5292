"""The cases, seeded operands and float64 references that tests/test_conv_f32_cases_cpu.py and tests/test_hip_conv_f32.py
share (torch on the CPU only): the fp32 conv kernels of skoots_amd/csrc/conv3d_f32.hip.

A case is ``(B, out spatial, [(C, up)], cout, ksize)``: the layer's sources are concatenated along the channels, a source
with ``up`` is stored at half the output extent and read through a nearest upsample; ksize 3 has padding 1 and stride 1,
ksize 2 stride 2, ksize 1 stride 1.  Each case is the smallest shape that reaches the branch named next to it.

Two kinds of operands:

``integer``    activations uniform integers in [-2, 2], weights in {-1, 0, 1}, biases in [-4, 4].  v_mfma_f32_32x32x2_f32 is
               an fmaf chain, so as long as sum |x||w| + |b| stays below 2^24 every partial accumulation is an exact
               integer in ANY order: the kernel must equal the float64 conv bit for bit, and so must every GroupNorm
               partial row while the row's sum |r| and sum r^2 stay below 2^24 (tests/test_conv_f32_cases_cpu.py asserts
               both conditions from the reference alone).
``realistic``  activations randn, weights randn / sqrt(cin k^3), biases 0.1 randn: a unit-variance output.

The GroupNorm partial layout (include/skoots_hip.h, sk_conv3d_f32_num_blocks): row r of sample b holds, per quad of four
consecutive output channels, the sum and the sum of squares over the voxels [128 r, 128 r + 128) of the sample in
x-major order; the last row is ragged.
"""
import functools

import torch
import torch.nn.functional as F

ROW = 128                 # voxels per GroupNorm partial row

CASES = [
    # (B, out spatial, [(C, up)], cout, ksize)
    (2, (5, 6, 7), [(32, 0)], 32, 3),               # 210 voxels: one block, second half-tile partly masked, 2 rows
    (1, (9, 6, 7), [(32, 0)], 32, 3),               # 378 voxels: 3 rows (odd: the second block's second row does not
                                                    # exist); a 256-voxel block spans 7 x-planes
    (1, (3, 20, 16), [(32, 0)], 32, 3),             # a plane of 320 voxels: blocks start in mid-plane
    (1, (6, 8, 4), [(32, 0), (64, 1)], 64, 3),      # two sources, upsample, two cout tiles
    (1, (2, 4, 130), [(64, 0), (64, 1)], 64, 3),    # upsampled window, long z
    (1, (4, 5, 3), [(128, 0)], 128, 3),             # four cout tiles
    (1, (4, 6, 4), [(128, 0), (128, 1)], 128, 3),   # K = 6912
    (2, (3, 5, 4), [(32, 0)], 64, 2),               # stride 2
    (1, (5, 3, 9), [(128, 0)], 64, 1),              # 1x1x1
    (2, (6, 5, 4), [(32, 0)], 5, 1),                # the heads: cout % 32 != 0, no partials
    (1, (3, 5, 4), [(5, 0)], 32, 3),                # gather kernel, odd C
    (1, (4, 6, 4), [(3, 0), (32, 1)], 32, 3),       # gather kernel, two sources, upsample
]
TWO_SOURCE_CASE = CASES[3]
STRIDE2_CASE = CASES[7]


def case_id(case):
    B, osp, srcdef, cout, k = case
    return f"B{B}-{'x'.join(map(str, osp))}-" + "+".join(f"{c}{'u' if up else ''}" for c, up in srcdef) + f"-{cout}-k{k}"


def has_partials(case):
    return case[3] % 32 == 0


def source_shapes(case):
    """[(B, C, xs, ys, zs)]: the stored shape of every source, channels first"""
    B, osp, srcdef, _, k = case
    s = 2 if k == 2 else 1
    return [(B, c) + (tuple(v // 2 for v in osp) if up else tuple(v * s for v in osp)) for c, up in srcdef]


def _seed(case, kind):
    B, osp, srcdef, cout, k = case
    return 1000 * kind + 97 * B + 31 * osp[0] + 17 * osp[1] + 7 * osp[2] + 5 * cout + 3 * k + sum(c + up for c, up in srcdef)


def integer_operands(case):
    """(sources, weight, bias) float32, integer-valued: activations in [-2, 2], weights in {-1, 0, 1}, biases in [-4, 4]"""
    _, _, srcdef, cout, k = case
    g = torch.Generator().manual_seed(_seed(case, 1))
    srcs = [torch.randint(-2, 3, shp, generator=g).float() for shp in source_shapes(case)]
    cin = sum(c for c, _ in srcdef)
    w = torch.randint(-1, 2, (cout, cin, k, k, k), generator=g).float()
    b = torch.randint(-4, 5, (cout,), generator=g).float()
    return srcs, w, b


def realistic_operands(case):
    """(sources, weight, bias) float32: randn, randn / sqrt(cin k^3), 0.1 randn"""
    _, _, srcdef, cout, k = case
    g = torch.Generator().manual_seed(_seed(case, 2))
    srcs = [torch.randn(shp, generator=g) for shp in source_shapes(case)]
    cin = sum(c for c, _ in srcdef)
    w = torch.randn((cout, cin, k, k, k), generator=g) / (cin * k ** 3) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return srcs, w, b


def assemble(case, srcs):
    """The conv's input (B, cin, ...) in the sources' dtype: upsampled sources through a nearest upsample, concatenated"""
    xs = [F.interpolate(t, scale_factor=2, mode="nearest") if up else t for t, (_, up) in zip(srcs, case[2])]
    return torch.cat(xs, dim=1)


def conv(case, srcs, w, b):
    """F.conv3d of the assembled sources in the operands' dtype -> (B, cout, ox, oy, oz)"""
    k = case[4]
    x = assemble(case, srcs)
    return F.conv3d(x, w, b, padding=1) if k == 3 else F.conv3d(x, w, b, stride=k)


def conv64(case, srcs, w, b):
    return conv(case, [t.double() for t in srcs], w.double(), b.double())


def num_rows(case):
    ox, oy, oz = case[1]
    return (ox * oy * oz + ROW - 1) // ROW


def row_sums(y):
    """y (B, cout, ox, oy, oz) float64 -> (B, rows, cout / 4, 2): per 128-voxel row and channel quad, sum and sum of squares"""
    B, cout = y.shape[:2]
    v = y.reshape(B, cout, -1).transpose(1, 2)                      # (B, nvox, cout)
    n = v.shape[1]
    rows = (n + ROW - 1) // ROW
    v = F.pad(v, (0, 0, 0, rows * ROW - n)).reshape(B, rows, ROW, cout // 4, 4)
    return torch.stack([v.sum(dim=(2, 4)), (v * v).sum(dim=(2, 4))], dim=-1)


def half_rounded(t):
    """t with every element rounded to fp16, as float64"""
    return t.half().double()


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    ref = ref.double()
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1.0)).item()


@functools.lru_cache(maxsize=None)
def _integer(idx):
    srcs, w, b = integer_operands(CASES[idx])
    y = conv64(CASES[idx], srcs, w, b)
    rows = row_sums(y) if has_partials(CASES[idx]) else None
    return srcs, w, b, y, rows


@functools.lru_cache(maxsize=None)
def _realistic(idx):
    case = CASES[idx]
    srcs, w, b = realistic_operands(case)
    y = conv64(case, srcs, w, b)
    e32 = rel_err(conv(case, srcs, w, b), y)
    e16 = rel_err(conv(case, [half_rounded(t) for t in srcs], half_rounded(w), b.double()), y)
    rows = row_sums(y) if has_partials(case) else None
    return srcs, w, b, y, rows, e32, e16


def integer_expected(case):
    """(sources, weight, bias, float64 conv, float64 partial rows or None) of a case; computed once, not to be modified"""
    return _integer(CASES.index(case))


def realistic_expected(case):
    """(sources, weight, bias, float64 conv, float64 partial rows or None, e32, e16): e32 torch's fp32 CPU conv against
    float64, e16 the float64 conv of fp16-rounded activations and weights against float64, both over
    max(1, max |ref|); computed once, not to be modified"""
    return _realistic(CASES.index(case))
