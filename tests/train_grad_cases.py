"""The cases, plan mirror, seeded operands and float64 references that tests/test_train_grad_cases_cpu.py and
tests/test_hip_train_grad_exact.py share (torch on the CPU only): the conv gradients of the training step in
skoots_amd/csrc/train.hip -- the weight gradient behind sk_train_conv_wgrad, sk_train_conv_wgrad_f16 and
sk_train_stem_wgrad_f16, and the 16-bit data gradient sk_train_pack_weight + sk_conv3d (+ sk_train_interleave2).

A case is ``(B, out spatial, [(C, up)], cout, ksize)``, the tuple of BWD_CASES in tests/test_hip_train.py: the layer's sources
are concatenated along the channels, a source with ``up`` is stored at half the output extent and read through a nearest
upsample; ksize 3 has padding 1 and stride 1, ksize 2 stride 2, ksize 1 stride 1.  CASES holds, next to every case, the
instantiation it runs through each entry point -- what ``route`` returns for it, which is the library's own answer: wgrad_route
of skoots_amd/csrc/train.hip, the one function the three entry points ask, through the host-only sk_train_conv_wgrad_route.
tests/test_train_grad_cases_cpu.py asserts every column and that together they cover every name
sk_train_conv_wgrad_route_name lists.  ``plan``, ``y_columns`` and ``workspace_floats`` stay an independent restatement of the
route's numbers, compared with the library's.

Entries and route names:
``fp32``      sk_train_conv_wgrad:       ``wgrad_stem<false>`` (one plain 1-channel source, ksize 3), ``wgrad<9>`` ``wgrad<8>``
              ``wgrad<1>`` (wgrad_kernel<NT>, NT taps a wave: ksize 3, 2, 1)
``f16``       sk_train_conv_wgrad_f16:   ``wgrad16x`` (x-marching 16 x 16 footprints), ``wgrad16y`` (y-walking strip ring),
              ``wgrad16t<9|8|1>`` (whole 64-byte lines through LDS), ``wgrad16<9|8|1>`` (16-bit buffer loads); the first
              three need a zero page and channel counts % 32 == 0
``stem_f16``  sk_train_stem_wgrad_f16:   ``wgrad_stem16`` (Z % 16 == 0) or ``wgrad_stem<true>``

Operands.  Sources are integers in [-2, 2], dy is in {-1, 0, 1} with half of the voxels zero; the device dy is
dy * 2^SCALE_K with dy_scale = [2^SCALE_K, 2^-SCALE_K, .], still a small integer of either 16-bit type.  Every product is an
exact integer, the MFMAs accumulate in fp32 and wgrad_reduce_kernel sums the chunk rows in double, so while
max |x| * sum |dy16| stays below 2^24 every partial sum is exact in ANY order and the kernels must produce the float64
gradients bit for bit.  The stem's image is an fp32 operand of sk_train_conv_wgrad and sk_train_stem_wgrad_f16 (the latter
multiplies it as a 16-bit value plus the 16-bit rounding of the remainder): for those two entries the small stem cases use
``a + j 2^-10`` (a in [-2, 2], j in [-3, 3]) -- twelve significant bits, more than either 16-bit type holds in one value, all of
them inside value + remainder --, and the bounds are counted in units of 2^-10.
"""
import functools

import torch
import torch.nn.functional as F

LIMIT = 2 ** 24
SCALE_K = 2                      # the device dy is dy * 2^SCALE_K
EXACT_INT = {"fp16": 2048, "bf16": 256}   # |integer| up to here is exact in the type (11 and 8 significant bits)
FINE_UNIT = 2.0 ** -10           # the stem image's grain for the fp32-image entries
FINE_VOXELS = 4096               # ... on cases of at most this many voxels (B x volume); larger ones keep integer images

ENTRIES = ("fp32", "f16", "stem_f16")


# ---------------------------------------------------------------------------------------------- the plan mirror
def cin_of(case):
    return sum(c for c, _ in case[2])


def is_stem(case):
    """one plain 1-channel source under a 3x3x3 conv: what sk_train_conv_wgrad sends to wgrad_stem_kernel"""
    _, _, srcdef, _, k = case
    return k == 3 and len(srcdef) == 1 and srcdef[0] == (1, 0)


def plan(case, entry="f16"):
    """The chunking of wgrad_route (skoots_amd/csrc/train.hip), voxel chunks and x-marching footprints, as `entry` runs it
    -> dict(nchunk, nchunk_b, chunk, ngroup, nchunk_x, nxs, xseg, empty).  The 16-bit entry points round ``chunk`` up to whole
    16-voxel steps AFTER the chunk count was fixed: sk_train_conv_wgrad_f16 ("f16") always, sk_train_stem_wgrad_f16
    ("stem_f16") where Z % 16 == 0 (wgrad_stem16; wgrad_stem<true> keeps the plan's chunk), sk_train_conv_wgrad ("fp32")
    never.  ``empty`` lists the chunk indices (b * nchunk_b + cb) that then start at or past the volume's end.  The counts
    and so the workspace size are the same for every entry."""
    assert entry in ENTRIES
    rounded = entry == "f16" or (entry == "stem_f16" and case[1][2] % 16 == 0)
    B, (ox, oy, oz), _, cout, k = case
    cin = cin_of(case)
    ncot, ncit = (cout + 31) // 32, (cin + 31) // 32
    ngroup = 3 if k == 3 else 1
    nvox = ox * oy * oz
    want = max(1, 4096 // (ncot * ncit * ngroup * B))
    c = max(512, (nvox + want - 1) // want)
    c = (c + 1) & ~1
    nchunk_b = (nvox + c - 1) // c
    if rounded:
        c = (c + 15) & ~15
    empty = [b * nchunk_b + cb for b in range(B) for cb in range(nchunk_b) if cb * c >= nvox]
    nchunk_x = nxs = xseg = 0
    if k == 3 and oy % 16 == 0 and oz % 16 == 0 and cout % 32 == 0 and cin % 32 == 0:
        wg = B * (oy // 16) * (oz // 16) * (cout // 32) * (cin // 32)
        s = max(1, min((1024 + wg - 1) // wg, ox // 8))
        xseg = (ox + s - 1) // s
        nxs = (ox + xseg - 1) // xseg
        nchunk_x = B * (oy // 16) * (oz // 16) * nxs
    return dict(nchunk=B * nchunk_b, nchunk_b=nchunk_b, chunk=c, ngroup=ngroup, nchunk_x=nchunk_x, nxs=nxs, xseg=xseg,
                empty=empty)


def y_columns(case):
    """wgrad16y_kernel deals columns (x, 16-voxel z block) out to the plan's chunks: (columns, columns a chunk, the chunk
    indices left without a column)"""
    B, (ox, _, oz), _, _, _ = case
    nb = plan(case)["nchunk_b"]
    ncol = ox * (oz // 16)
    per = (ncol + nb - 1) // nb
    return ncol, per, [b * nb + cb for b in range(B) for cb in range(nb) if cb * per >= ncol]


def workspace_floats(case):
    """sk_train_conv_wgrad_workspace_floats: max(nchunk, nchunk_x) rows of (cout cin k^3 + cout) floats"""
    _, _, _, cout, k = case
    p = plan(case)
    return max(p["nchunk"], p["nchunk_x"]) * (cout * cin_of(case) * k ** 3 + cout)


def accepts(case, entry):
    """whether the entry point takes the case at all (sk_train_stem_wgrad_f16: the stem layer, 1 -> 32 channels)"""
    return entry != "stem_f16" or (is_stem(case) and case[3] == 32)


def library_route(case, entry, zero_page=False, twin=False):
    """sk_train_conv_wgrad_route (host only: no GPU) for a case as the entry point would launch it -> the filled
    skoots_amd._ffi.WgradRoute"""
    from skoots_amd import _ffi
    assert entry in ENTRIES and accepts(case, entry)
    B, (ox, oy, oz), srcdef, cout, k = case
    arr = (_ffi.ConvSrc * len(srcdef))()
    for a, (c, up) in zip(arr, srcdef):
        a.data, a.affine, a.c, a.upsample = None, None, c, up
    r = _ffi.WgradRoute()
    fn = getattr(_ffi.lib, "sk_train_conv_wgrad_route" + ("_bf16" if twin else ""))
    _ffi.check(fn(ENTRIES.index(entry), arr, len(srcdef), B, ox, oy, oz, cout, k, int(zero_page), r))
    return r


def route(case, entry, zero_page=False):
    """The instantiation an entry point launches: wgrad_route of skoots_amd/csrc/train.hip, asked through
    sk_train_conv_wgrad_route"""
    return library_route(case, entry, zero_page).name.decode()


def library_names(entry, twin=False):
    """sk_train_conv_wgrad_route_name until NULL: every kernel the entry point can reach in the release build"""
    from skoots_amd import _ffi
    fn = getattr(_ffi.lib, "sk_train_conv_wgrad_route_name" + ("_bf16" if twin else ""))
    names = []
    while fn(ENTRIES.index(entry), len(names)) is not None:
        names.append(fn(ENTRIES.index(entry), len(names)).decode())
    return names


# literal, and held equal to what sk_train_conv_wgrad_route_name lists (tests/test_train_grad_cases_cpu.py): a kernel added
# to the library's tables without a case below fails on the CPU
REACHABLE = {
    "fp32": {"wgrad_stem<false>", "wgrad<9>", "wgrad<8>", "wgrad<1>"},
    "f16": {"wgrad16x", "wgrad16y", "wgrad16t<9>", "wgrad16t<8>", "wgrad16t<1>", "wgrad16<9>", "wgrad16<8>", "wgrad16<1>"},
    "stem_f16": {"wgrad_stem16", "wgrad_stem<true>"},
}


def family(name):
    """wgrad_stem<false> and wgrad_stem<true> are the two entry points' own; the others by template"""
    return name if name.startswith("wgrad_stem") else name.split("<")[0]


# ---------------------------------------------------------------------------------------------- the case table
S1, S32, S64, S128 = [(1, 0)], [(32, 0)], [(64, 0)], [(128, 0)]
U32, U64 = [(32, 0), (32, 1)], [(64, 0), (64, 1)]
CASES = [
    # (case, fp32 route, f16 route with a zero page, f16 route without, stem_f16 route or None)
    # ---- the stem: 1 -> 32, ksize 3
    ((2, (7, 6, 5), S1, 32, 3), "wgrad_stem<false>", "wgrad16<9>", "wgrad16<9>", "wgrad_stem<true>"),   # batch 2, odd extents
    ((1, (9, 8, 9), S1, 32, 3), "wgrad_stem<false>", "wgrad16<9>", "wgrad16<9>", "wgrad_stem<true>"),   # 648 voxels: 2 chunks
    ((2, (5, 6, 16), S1, 32, 3), "wgrad_stem<false>", "wgrad16<9>", "wgrad16<9>", "wgrad_stem16"),      # batch 2
    ((1, (9, 8, 16), S1, 32, 3), "wgrad_stem<false>", "wgrad16<9>", "wgrad16<9>", "wgrad_stem16"),      # 1152 voxels: 3 chunks
    # 170 chunks an item of 514 voxels, run as 528: the chunks 166 .. 169 of every item start past its 87216 voxels
    ((8, (79, 69, 16), S1, 32, 3), "wgrad_stem<false>", "wgrad16<9>", "wgrad16<9>", "wgrad_stem16"),
    # ---- ksize 3, whole 32-channel tiles: no special plane geometry
    ((2, (6, 5, 4), S32, 32, 3), "wgrad<9>", "wgrad16t<9>", "wgrad16<9>", None),     # batch 2
    ((1, (6, 8, 4), U32, 32, 3), "wgrad<9>", "wgrad16t<9>", "wgrad16<9>", None),     # decoder concat: second half upsampled
    ((1, (4, 6, 4), U64, 64, 3), "wgrad<9>", "wgrad16t<9>", "wgrad16<9>", None),     # 2 cout tiles x 4 cin tiles
    ((1, (33, 20, 9), S32, 32, 3), "wgrad<9>", "wgrad16t<9>", "wgrad16<9>", None),   # 5940 voxels: 12 chunks
    ((1, (6, 6, 16), S32, 32, 3), "wgrad<9>", "wgrad16t<9>", "wgrad16<9>", None),    # z % 16 == 0 but y % 4 != 0
    # 42 chunks an item of 514 voxels, run as 528: chunk 41 of either item starts at 21648 > 21560 voxels
    ((2, (49, 44, 10), S128, 128, 3), "wgrad<9>", "wgrad16t<9>", "wgrad16<9>", None),
    # ---- ksize 3, ragged channels (never whole lines)
    ((2, (5, 6, 7), [(40, 0)], 5, 3), "wgrad<9>", "wgrad16<9>", "wgrad16<9>", None),   # cout 5, cin 40: ragged second cin tile
    # ---- ksize 3, z % 16 == 0 and y % 4 == 0: the strip ring
    ((2, (5, 8, 16), S32, 32, 3), "wgrad<9>", "wgrad16y", "wgrad16<9>", None),       # batch 2
    ((1, (4, 12, 32), U32, 32, 3), "wgrad<9>", "wgrad16y", "wgrad16<9>", None),      # an upsampled half, two z blocks
    ((1, (40, 8, 16), S64, 64, 3), "wgrad<9>", "wgrad16y", "wgrad16<9>", None),      # 5120 voxels: 10 chunks, 2 x 2 tiles
    ((1, (2, 40, 16), S32, 32, 3), "wgrad<9>", "wgrad16y", "wgrad16<9>", None),      # 3 chunks for 2 columns: the third has none
    # ---- ksize 3, y % 16 == 0 and z % 16 == 0: the x-marching kernel
    ((2, (5, 16, 16), S32, 32, 3), "wgrad<9>", "wgrad16x", "wgrad16<9>", None),      # batch 2: 2 chunks in a round of 8
    ((1, (12, 32, 16), U32, 32, 3), "wgrad<9>", "wgrad16x", "wgrad16<9>", None),     # two y footprints, an upsampled half
    ((1, (20, 16, 32), S64, 64, 3), "wgrad<9>", "wgrad16x", "wgrad16<9>", None),     # two z footprints, two x segments, 2 x 2 tiles
    ((1, (6, 16, 16), [(32, 0), (64, 1)], 64, 3), "wgrad<9>", "wgrad16x", "wgrad16<9>", None),   # three cin tiles of two sources
    # one plane: 12 footprints against the plan's 6 chunks -- the x kernel's rows size the workspace, which ends where its
    # last row ends, and 12 chunks are a launch round and a half: the surplus workgroups sit right in front of the tail
    ((1, (1, 48, 64), S32, 32, 3), "wgrad<9>", "wgrad16x", "wgrad16<9>", None),
    ((2, (1, 32, 48), S32, 32, 3), "wgrad<9>", "wgrad16x", "wgrad16<9>", None),      # ... with batch 2: 12 against 6 again
    # ---- ksize 2: the stride-2 down convs
    ((2, (3, 4, 2), S32, 64, 2), "wgrad<8>", "wgrad16t<8>", "wgrad16<8>", None),     # batch 2, two cout tiles
    ((1, (9, 8, 9), S32, 64, 2), "wgrad<8>", "wgrad16t<8>", "wgrad16<8>", None),     # 648 voxels: 2 chunks
    ((2, (3, 5, 2), S64, 128, 2), "wgrad<8>", "wgrad16t<8>", "wgrad16<8>", None),    # 4 cout tiles x 2 cin tiles
    ((1, (3, 4, 5), [(24, 0)], 5, 2), "wgrad<8>", "wgrad16<8>", "wgrad16<8>", None),   # ragged: cout 5, cin 24
    # ---- ksize 1
    ((1, (5, 3, 4), S128, 64, 1), "wgrad<1>", "wgrad16t<1>", "wgrad16<1>", None),    # pointwise reducer: 2 x 4 tiles
    ((2, (9, 9, 8), S64, 32, 1), "wgrad<1>", "wgrad16t<1>", "wgrad16<1>", None),     # batch 2, 648 voxels: 2 chunks an item
    ((2, (6, 5, 4), S32, 5, 1), "wgrad<1>", "wgrad16<1>", "wgrad16<1>", None),       # the heads: cout 5
    ((2, (9, 9, 8), [(40, 0)], 5, 1), "wgrad<1>", "wgrad16<1>", "wgrad16<1>", None),   # ... on cin 40, 2 chunks an item
]
ALL = [row[0] for row in CASES]
# the cases whose plan, after the 16-rounding, has chunks that start past the volume (the mirror decides: asserted on the
# CPU); every voxel-chunked 16-bit route has one: wgrad_stem16 and wgrad16<9> (either), wgrad16t<9> and wgrad16<9> (the second)
EMPTY_CHUNK_CASES = [(8, (79, 69, 16), S1, 32, 3), (2, (49, 44, 10), S128, 128, 3)]
assert all(c in ALL for c in EMPTY_CHUNK_CASES)


def named(case, entry, zero_page=False):
    """the route written next to a case in CASES (None: the entry does not take it)"""
    row = CASES[ALL.index(case)]
    return {"fp32": row[1], "f16": row[2] if zero_page else row[3], "stem_f16": row[4]}[entry]


def runs():
    """every (case, entry, zero_page) the GPU test runs"""
    out = []
    for case in ALL:
        out.append((case, "fp32", False))
        out.append((case, "f16", True))
        out.append((case, "f16", False))
        if accepts(case, "stem_f16"):
            out.append((case, "stem_f16", False))
    return out


def case_id(case):
    B, osp, srcdef, cout, k = case
    return f"B{B}-{'x'.join(map(str, osp))}-" + "+".join(f"{c}{'u' if up else ''}" for c, up in srcdef) + f"-{cout}-k{k}"


def source_shapes(case):
    """[(B, C, xs, ys, zs)]: the stored shape of every source, channels first"""
    B, osp, srcdef, _, k = case
    s = 2 if k == 2 else 1
    return [(B, c) + (tuple(v // 2 for v in osp) if up else tuple(v * s for v in osp)) for c, up in srcdef]


def _seed(case, kind):
    B, osp, srcdef, cout, k = case
    return 1000 * kind + 97 * B + 31 * osp[0] + 17 * osp[1] + 7 * osp[2] + 5 * cout + 3 * k + sum(c + up for c, up in srcdef)


# ---------------------------------------------------------------------------------------------- operands and references
def has_fine_image(case):
    """the stem cases whose fp32-image entries (fp32, stem_f16) get the 2^-10-grained image"""
    B, (ox, oy, oz), _, _, _ = case
    return is_stem(case) and B * ox * oy * oz <= FINE_VOXELS


def integer_operands(case):
    """(sources, dy) float32, channels first: sources integers in [-2, 2], dy (B, cout, ox, oy, oz) in {-1, 0, 1}, half of it
    thinned to zero"""
    B, osp, _, cout, _ = case
    g = torch.Generator().manual_seed(_seed(case, 1))
    srcs = [torch.randint(-2, 3, shp, generator=g).float() for shp in source_shapes(case)]
    shp = (B, cout) + tuple(osp)
    dy = torch.randint(-1, 2, shp, generator=g).float() * (torch.rand(shp, generator=g) < 0.5).float()
    return srcs, dy


def fine_image(case):
    """the stem image a + j 2^-10, a integer in [-2, 2], j in [-3, 3] (float32, (B, 1, X, Y, Z))"""
    assert has_fine_image(case)
    g = torch.Generator().manual_seed(_seed(case, 2))
    shp = source_shapes(case)[0]
    return torch.randint(-2, 3, shp, generator=g).float() + torch.randint(-3, 4, shp, generator=g).float() * FINE_UNIT


def assemble(case, srcs):
    """The conv's input (B, cin, ...) in the sources' dtype: upsampled sources through a nearest upsample, concatenated"""
    xs = [F.interpolate(t, scale_factor=2, mode="nearest") if up else t for t, (_, up) in zip(srcs, case[2])]
    return torch.cat(xs, dim=1)


def wgrad64(case, srcs, dy):
    """float64 (dweight (cout, cin, k, k, k), dbias (cout)) of the conv of `case`: per tap one matrix product of dy with the
    input shifted by the tap, dW[co][ci][tap] = sum_{b, v} dy[b, co, v] x[b, ci, in(v, tap)]"""
    B, (ox, oy, oz), _, cout, k = case
    x = assemble(case, [t.double() for t in srcs])
    cin = x.shape[1]
    if k == 3:
        x = F.pad(x, (1, 1, 1, 1, 1, 1))
    d = dy.double().reshape(B, cout, -1)
    dw = torch.empty((cout, cin, k, k, k), dtype=torch.float64)
    for tx in range(k):
        for ty in range(k):
            for tz in range(k):
                xs = x[:, :, tx:tx + ox, ty:ty + oy, tz:tz + oz] if k == 3 else x[:, :, tx::k, ty::k, tz::k]
                dw[:, :, tx, ty, tz] = torch.einsum("bov,bcv->oc", d, xs.reshape(B, cin, -1))
    return dw, d.sum(dim=(0, 2))


@functools.lru_cache(maxsize=None)
def _expected(idx, fine):
    case = ALL[idx]
    srcs, dy = integer_operands(case)
    if fine:
        srcs = [fine_image(case)]
    dw, db = wgrad64(case, srcs, dy)
    return srcs, dy, dw, db


def uses_fine_image(case, entry):
    return has_fine_image(case) and entry in ("fp32", "stem_f16")


def expected(case, entry):
    """(sources, dy, float64 dweight, float64 dbias) for a case as `entry` sees it; computed once per (case, image kind), not
    to be modified"""
    return _expected(ALL.index(case), uses_fine_image(case, entry))


# ---------------------------------------------------------------------------------------------- sk_train_pack_weight
# (Co, Ci, ksize) of the layer weight (Co, Ci, k, k, k) packed with transposed = 0 against sk_conv3d_pack_weight_host
PACK_FORWARD = [(32, 32, 3), (32, 64, 3),              # ksize 3, cout 32: the 16x16x32 fragment order
                (64, 32, 3), (64, 64, 3), (128, 64, 3), (128, 128, 3),
                (64, 32, 2), (128, 64, 2), (32, 32, 1), (32, 16, 1), (64, 128, 1), (128, 64, 1)]
# (B, out spatial, Co, Ci, ksize, [(c_lo, c_n)]): transposed = 1, the data gradient of input channels [c_lo, c_lo + c_n) as
# sk_conv3d of dy (B, ox, oy, oz, Co) with the packed operator: the whole input, each half of a two-source layer, a range that
# does not start at 0
DGRAD_CASES = [
    (2, (5, 7, 6), 32, 64, 3, [(0, 64), (0, 32), (32, 32)]),
    (1, (4, 5, 6), 64, 128, 3, [(0, 128), (64, 64), (32, 32)]),
    (1, (3, 4, 5), 128, 96, 3, [(0, 64), (64, 32), (32, 64)]),
    (2, (4, 5, 6), 64, 128, 1, [(0, 128), (0, 64), (64, 64), (96, 32)]),
    (1, (5, 3, 7), 32, 64, 1, [(0, 64), (32, 32)]),
]
# (B, coarse spatial, Co, Ci): transposed = 2, the stride-2 conv Ci -> Co (ksize 2) whose data gradient (B, 2cx, 2cy, 2cz, Ci)
# is eight pointwise products interleaved
DGRAD2_CASES = [(2, (3, 5, 3), 64, 32), (1, (3, 3, 5), 128, 64), (1, (2, 3, 3), 32, 32)]


def pack_forward_weight(Co, Ci, k):
    """a weight every element of which either 16-bit type holds: m / 8, m integer in [-100, 100]"""
    g = torch.Generator().manual_seed(7 * Co + 3 * Ci + k)
    return torch.randint(-100, 101, (Co, Ci, k, k, k), generator=g).float() / 8


@functools.lru_cache(maxsize=None)
def _dgrad(idx):
    B, osp, Co, Ci, k, _ = DGRAD_CASES[idx]
    g = torch.Generator().manual_seed(500 + 13 * idx)
    shp = (B, Co) + tuple(osp)
    dy = torch.randint(-1, 2, shp, generator=g).float() * (torch.rand(shp, generator=g) < 0.5).float()
    w = torch.randint(-1, 2, (Co, Ci, k, k, k), generator=g).float()
    dx = F.conv_transpose3d(dy.double(), w.double(), padding=1 if k == 3 else 0)
    return dy, w, dx


def dgrad_expected(idx):
    """(dy (B, Co, ...) in {-1, 0, 1}, half of it zero; weight (Co, Ci, k, k, k) in {-1, 0, 1}, random and so without any
    symmetry; float64 data gradient (B, Ci, ...) = conv_transpose3d) of DGRAD_CASES[idx]; computed once, not to be modified"""
    return _dgrad(idx)


@functools.lru_cache(maxsize=None)
def _dgrad2(idx):
    B, csp, Co, Ci = DGRAD2_CASES[idx]
    g = torch.Generator().manual_seed(900 + 13 * idx)
    shp = (B, Co) + tuple(csp)
    dy = torch.randint(-1, 2, shp, generator=g).float() * (torch.rand(shp, generator=g) < 0.5).float()
    w = torch.randint(-1, 2, (Co, Ci, 2, 2, 2), generator=g).float()
    dx = F.conv_transpose3d(dy.double(), w.double(), stride=2)
    return dy, w, dx


def dgrad2_expected(idx):
    """the same for DGRAD2_CASES[idx]: dy (B, Co, cx, cy, cz), weight (Co, Ci, 2, 2, 2), float64 dx (B, Ci, 2cx, 2cy, 2cz) =
    conv_transpose3d with stride 2"""
    return _dgrad2(idx)
