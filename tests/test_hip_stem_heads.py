"""GPU tests of the first and last kernels of every inference tile -- the stem (sk_conv3d_stem, _raw, _apply, _apply_split,
_apply_mix8, sk_train_stem_fwd_f16) and the heads (sk_heads, sk_heads_split, sk_train_heads_fwd_f16 / _wgrad_f16) --
each against a float64 reference of the same operation, called through the C ABI directly.

The network tests bound these kernels only through several other layers (1e-3 max-abs on the output), while each of them
is designed to "exact products, fp32 accumulation", about 1e-6 relative.  Every floating-point bound below is derived from
the kernel's stated arithmetic, per voxel, from the operands themselves (sums of |x||w|), with u = 2^-24 the unit
roundoff of fp32:

  * weights split w = hi + lo, hi = fp16(w), lo = fp16(w - hi): the products with fp16 operands are exact; what the pair
    misses, |w - hi - lo|, is computed exactly from w (at most max(2^-22 |w|, 2^-25));
  * a sum of n terms accumulated in fp32, in any order, is off by at most (n - 1) u sum |term| (each addition rounds
    once, and every partial sum is bounded by sum |term|);
  * fmaf rounds once; __expf(x) = exp2(x log2 e) carries (|x| + 2) u relative (the rounded product plus v_exp_f32's own
    ulp), rcpf 2 u, every other fp32 operation u;
  * silu' lies in [-0.1, 1.1], tanh' in [0, 1], sigmoid' in [0, 1/4]: an input error e moves them by at most 1.1 e, e, e / 4;
  * an fp16 store adds half an fp16 ulp of the stored value; a split pair [hi | lo] max(2^-22 |x|, 2^-25).

Exact tests (integer operands, delta-tap weights) need no bound: they pin layouts, tap order, frames, channel rows and
the partial sums bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24            # fp32 unit roundoff
SENT = 7.0                # sentinel fill: no stem / heads output can hold it where the tests put it


@pytest.fixture(scope="module")
def ffi():
    from skoots_amd import _ffi
    return _ffi


def _st():
    from skoots_amd import _ffi
    return _ffi.stream_ptr(torch.device(DEV))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


MEASURED = {}   # largest err / bound seen per check (what the bounds leave unused; read by a measuring run)


def _within(err, bnd, key, msg):
    """assert err <= bnd elementwise; remember the largest ratio under `key`."""
    ratio = float((err / bnd).max()) if err.numel() else 0.0
    MEASURED[key] = max(MEASURED.get(key, 0.0), ratio)
    assert (err <= bnd).all(), f"{msg}: {ratio:.3g} x bound"


def _ulp16(a):
    """fp16 ulp at magnitude |a| (float64 tensor): 2^(e - 10) for |a| in [2^e, 2^(e+1)), 2^-24 in the subnormal range."""
    m, e = torch.frexp(a.abs().clamp_min(2.0 ** -14))
    return torch.ldexp(torch.ones_like(a), (e - 11).to(torch.int32))


def _split_err(w):
    """|w - hi - lo| of the kernels' weight split, exactly (float64), and lo itself."""
    hi = w.float().half().double()
    lo = (w.float() - w.float().half().float()).half().double()
    return (w.double() - hi - lo).abs(), lo


# ============================================================================================ stem
def _stem_rows(Yt, Zt):
    r = 40 * 1024 // (3 * (Zt + 2) * 2) - 2
    r = min(max(min(r, 150), 1), Yt)
    n = -(-Yt // r)
    return -(-Yt // n)


def _norm_rule(vol, o, tile, mean, std):
    """The kernel's written rule fp16(fp16(x - mean) / std), fp32 mean / std, zero frame and zero overhang.
    vol: (X, Y, Z) float16 numpy -> (Xt + 2, Yt + 2, Zt + 2) float16 numpy."""
    x, y, z = o
    Xt, Yt, Zt = tile
    crop = vol[x:x + Xt, y:y + Yt, z:z + Zt].astype(np.float32)
    s = (crop - np.float32(mean)).astype(np.float16).astype(np.float32)
    v = (s / np.float32(std)).astype(np.float16)
    out = np.zeros((Xt + 2, Yt + 2, Zt + 2), np.float16)
    out[1:1 + v.shape[0], 1:1 + v.shape[1], 1:1 + v.shape[2]] = v
    return out


def _norm_torch(vol, o, tile, mean, std):
    """eval.py:139 in torch on the CPU: crop.sub(mean).div(std) on the fp16 crop, zero-padded to the framed tile."""
    x, y, z = o
    Xt, Yt, Zt = tile
    v = vol[x:x + Xt, y:y + Yt, z:z + Zt].sub(mean).div(std)
    out = torch.zeros((Xt + 2, Yt + 2, Zt + 2), dtype=torch.float16)
    out[1:1 + v.shape[0], 1:1 + v.shape[1], 1:1 + v.shape[2]] = v
    return out


def _org(origins):
    return (C.c_int32 * (3 * len(origins)))(*[int(v) for o in origins for v in o])


def _stem_stats(ffi, vol_d, origins, tile, mean, std, wt, bias, raw=False):
    """sk_conv3d_stem (or sk_conv3d_stem_raw): -> (workspace, partial[, raw out])."""
    B = len(origins)
    Xt, Yt, Zt = tile
    X, Y, Z = vol_d.shape
    nblk = ffi.lib.sk_conv3d_stem_num_blocks(Xt, Yt, Zt)
    ws_bytes = ffi.lib.sk_conv3d_stem_workspace_bytes(B, Xt, Yt, Zt)
    ws = torch.full((ws_bytes // 2,), SENT, dtype=torch.float16, device=DEV)
    partial = torch.full((B, nblk, 8, 2), SENT, dtype=torch.float32, device=DEV)
    if raw:
        out = torch.full((B, Xt, Yt, Zt, 32), SENT, dtype=torch.float16, device=DEV)
        ffi.check(ffi.lib.sk_conv3d_stem_raw(_ptr(vol_d), X, Y, Z, _org(origins), B, Xt, Yt, Zt, mean, std, _ptr(wt),
                                             _ptr(bias), 32, _ptr(out), _ptr(partial), _ptr(ws), ws_bytes, _st()))
        torch.cuda.synchronize()
        return ws, partial, out
    ffi.check(ffi.lib.sk_conv3d_stem(_ptr(vol_d), X, Y, Z, _org(origins), B, Xt, Yt, Zt, mean, std, _ptr(wt), _ptr(bias), 32,
                                     _ptr(partial), _ptr(ws), ws_bytes, _st()))
    torch.cuda.synchronize()
    return ws, partial


def _stem_apply(ffi, mode, ws, tile, B, wt, bias, aff):
    Xt, Yt, Zt = tile
    fn = {1: ffi.lib.sk_conv3d_stem_apply, 3: ffi.lib.sk_conv3d_stem_apply_split, 4: ffi.lib.sk_conv3d_stem_apply_mix8}[mode]
    out = torch.full((B, Xt, Yt, Zt, 32 if mode == 1 else 64), SENT, dtype=torch.float16, device=DEV)
    ffi.check(fn(B, Xt, Yt, Zt, _ptr(wt), _ptr(bias), _ptr(aff), _ptr(out), 32, _ptr(ws), _st()))
    torch.cuda.synchronize()
    return out


def _patches(framed):
    """(Xt + 2, Yt + 2, Zt + 2) -> (Xt, Yt, Zt, 27), tap (dx * 3 + dy) * 3 + dz."""
    Xt, Yt, Zt = (s - 2 for s in framed.shape)
    return torch.stack([framed[dx:dx + Xt, dy:dy + Yt, dz:dz + Zt] for dx in range(3) for dy in range(3) for dz in range(3)],
                       dim=-1)


def _block_sums(v, rows):
    """v (Xt, Yt, Zt, 32) -> per stem workgroup (x plane, y chunk of `rows`) and channel quad: (Xt * nyc, 8)."""
    Xt, Yt = v.shape[0], v.shape[1]
    chunks = [v[:, y0:y0 + rows].sum(dim=(1, 2)) for y0 in range(0, Yt, rows)]       # each (Xt, 32)
    s = torch.stack(chunks, dim=1)                                                      # (Xt, nyc, 32)
    return s.reshape(Xt * len(chunks), 8, 4).sum(dim=-1)


def _stem_weights(seed):
    """The stem of a random-init network (unet.random_state_dict's recipe): weight (32, 1, 3, 3, 3), bias, gamma, beta."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand((32, 1, 3, 3, 3), generator=g) * 2 - 1) / 27 ** 0.5
    b = (torch.rand(32, generator=g) * 2 - 1) / 27 ** 0.5
    return w, b, torch.rand(32, generator=g) + 0.5, torch.rand(32, generator=g) * 0.6 - 0.3


def _tap_major(w):
    return w.reshape(32, 27).t().contiguous()


# ------------------------------------------------------------------------------------- A: delta taps
DELTA_CASES = [   # (image range, mean, std): fp16-representable means (where torch's CPU sub agrees) and others
    ("u8", 127.3, 73.91), ("u8", 127.5, 73.91), ("u16", 30000.7, 18000.3), ("u16", 30000.0, 18000.3)]


@pytest.mark.parametrize("rng,mean,std", DELTA_CASES)
def test_stem_delta_taps_exact(ffi, rng, mean, std):
    """Output channel c has weight 1 at tap c % 27, 0 elsewhere, bias 0: sk_conv3d_stem_raw's output channel c is then the
    normalised tile shifted by tap (dx, dy, dz) = divmod(c % 27) -- products with 1.0, fp16 in and out: BIT FOR BIT.
    Pins the tap order (dx*3+dy)*3+dz, the zero frame at every tile face and the zeros where a tile overhangs the volume
    by 1-3 voxels on every axis.  The normalisation is checked against the kernel's written rule fp16(fp16(x - mean) / std)
    (fp32 mean / std) always, and against torch's CPU crop.sub(mean).div(std) where mean is an fp16 value (torch's CPU
    sub rounds a Python scalar to the tensor's dtype first; the kernel does not).  All 256 uint8 values, and an image
    spanning the fp16 range up to 65504 (large inputs round differently in the subtraction)."""
    g = torch.Generator().manual_seed(len(rng) * 1000 + int(mean))
    X, Y, Z = 20, 25, 30
    if rng == "u8":
        vol = torch.randint(0, 256, (X, Y, Z), generator=g).to(torch.float16)
    else:
        vol = torch.randint(0, 65505, (X, Y, Z), generator=g).to(torch.float16)
    tile = (6, 10, 12)
    origins = [(0, 0, 0), (14, 15, 18), (15, 16, 19), (17, 18, 21), (16, 0, 20), (3, 17, 7)]   # exact far faces, overhang 1..3
    w = torch.zeros((27, 32))
    for c in range(32):
        w[c % 27, c] = 1.0
    bias = torch.zeros(32)
    wd, bd = w.to(DEV), bias.to(DEV)
    ws0, p0 = _stem_stats(ffi, vol.to(DEV), origins, tile, mean, std, wd, bd)
    ws, p2, raw = _stem_stats(ffi, vol.to(DEV), origins, tile, mean, std, wd, bd, raw=True)
    B = len(origins)
    Xt, Yt, Zt = tile
    framed = ws.cpu()[:B * (Xt + 2) * (Yt + 2) * (Zt + 2)].reshape(B, Xt + 2, Yt + 2, Zt + 2)
    assert torch.equal(ws0.cpu(), ws.cpu())
    seen = set()
    for b, o in enumerate(origins):
        want = torch.from_numpy(_norm_rule(vol.numpy(), o, tile, mean, std))
        assert torch.equal(framed[b].view(torch.int16), want.view(torch.int16)), f"tile {b}: normalisation != written rule"
        if float(torch.tensor(mean).half()) == mean:
            assert torch.equal(framed[b], _norm_torch(vol, o, tile, mean, std)), f"tile {b}: normalisation != torch"
        x, y, z = o
        seen.update(vol[x:x + Xt, y:y + Yt, z:z + Zt].unique().tolist())
        pt = _patches(want)                                   # (Xt, Yt, Zt, 27) fp16
        shifted = pt[..., torch.arange(32) % 27]
        assert torch.equal(raw[b].cpu().view(torch.int16), shifted.view(torch.int16)), f"tile {b}: tap layout"
    if rng == "u8":
        assert len(seen) == 256


# ------------------------------------------------------------------------------------- A: integer conv
@pytest.mark.parametrize("tile,B", [((3, 151, 20), 2), ((2, 40, 6), 3), ((1, 12, 2), 1)])
def test_stem_integer_conv_exact(ffi, tile, B):
    """mean 0, std 1, image and weights in {-1, 0, 1}, integer biases: the raw conv equals F.conv3d EXACTLY, and with every
    partial sum of squares below 2^24 (a workgroup holds rows * Zt <= 1520 voxels, |y| <= 29) the statistics partials
    (B, nblk, 8, 2) are exact integers: equal to the float64 per-(workgroup, channel quad) sums and sums of squares, and
    sk_conv3d_stem's bit-identical to sk_conv3d_stem_raw's.  The same operands through sk_train_stem_fwd_f16 (the framed
    copy of an fp32 image, MODE 2) and its bf16 twin (integers up to 256 are exact in bf16)."""
    Xt, Yt, Zt = tile
    g = torch.Generator().manual_seed(Yt * 10 + Zt)
    X, Y, Z = Xt + 5, Yt + 4, Zt + 3
    vol = torch.randint(-1, 2, (X, Y, Z), generator=g).to(torch.float16)
    origins = [(min(2 * b, X - 1), min(3 * b, Y - 1), min(b, Z - 1)) for b in range(B - 1)]
    origins.append((min(X - 1, X - Xt + 1), min(Y - 1, Y - Yt + 2), min(Z - 1, Z - Zt + 3)))   # overhangs
    w = torch.randint(-1, 2, (32, 1, 3, 3, 3), generator=g).float()
    bias = torch.randint(-2, 3, (32,), generator=g).float()
    wt, bd = _tap_major(w).to(DEV), bias.to(DEV)
    _, p0 = _stem_stats(ffi, vol.to(DEV), origins, tile, 0.0, 1.0, wt, bd)
    _, p2, raw = _stem_stats(ffi, vol.to(DEV), origins, tile, 0.0, 1.0, wt, bd, raw=True)
    assert torch.equal(p0, p2)
    framed = torch.stack([torch.from_numpy(_norm_rule(vol.numpy(), o, tile, 0.0, 1.0)) for o in origins]).double()
    want = F.conv3d(framed[:, None], w.double(), bias.double())                  # (B, 32, Xt, Yt, Zt), exact integers
    want = want.permute(0, 2, 3, 4, 1)
    assert torch.equal(raw.cpu().double(), want)
    rows = _stem_rows(Yt, Zt)
    for b in range(B):
        ps = torch.stack([_block_sums(want[b], rows), _block_sums(want[b] ** 2, rows)], dim=-1)
        assert torch.equal(p0[b].cpu().double(), ps), f"tile {b}: partials"
    # training stem: whole tiles of an fp32 image (no origins, no normalisation)
    img = framed[:, 1:-1, 1:-1, 1:-1].float().contiguous()
    for sfx, dt in (("", torch.float16), ("_bf16", torch.bfloat16)):
        nblk = getattr(ffi.lib, "sk_conv3d_stem_num_blocks" + sfx)(Xt, Yt, Zt)
        ws_bytes = getattr(ffi.lib, "sk_conv3d_stem_workspace_bytes" + sfx)(B, Xt, Yt, Zt)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        y16 = torch.full((B, Xt, Yt, Zt, 32), SENT, dtype=dt, device=DEV)
        pt = torch.full((B, nblk, 8, 2), SENT, device=DEV)
        imgd = img.to(DEV)
        ffi.check(getattr(ffi.lib, "sk_train_stem_fwd_f16" + sfx)(_ptr(imgd), B, Xt, Yt, Zt, _ptr(wt), _ptr(bd), _ptr(y16),
                                                                   _ptr(pt), _ptr(ws), ws_bytes, _st()))
        torch.cuda.synchronize()
        assert torch.equal(y16.cpu().double(), want), sfx
        assert torch.equal(pt, p2), sfx


# ------------------------------------------------------------------------------------- B: apply modes
def _stem_case_origins(vol_shape, tile, B, seed):
    """B distinct origins: the volume's corner, its far faces (exactly and with an overhang of 1-3 voxels where the tile
    allows one), then random interior ones."""
    X, Y, Z = vol_shape
    cand = [(0, 0, 0)]
    for k in range(4):
        cand.append(tuple(min(s - 1, s - t + k) for s, t in zip(vol_shape, tile)))
    cand.append((X - tile[0], 0, min(Z - 1, Z - tile[2] + 1)))
    g = torch.Generator().manual_seed(seed)
    while len(set(cand)) < B + 8:
        cand.append(tuple(int(torch.randint(0, max(1, s - t + 1), (1,), generator=g)) for s, t in zip(vol_shape, tile)))
    out = []
    for o in cand:
        if o not in out:
            out.append(o)
    return out[:B]


STEM_CASES = [   # (B, tile, volume)
    (1, (3, 12, 20), (9, 20, 30)),          # one y chunk
    (3, (2, 150, 20), (4, 160, 24)),        # exactly 150 rows
    (1, (1, 151, 22), (3, 153, 40)),        # Xt = 1, ragged second chunk (76 + 75)
    (3, (3, 152, 6), (5, 154, 9)),          # two chunks of 76; Zt % 4 == 2, rows * Zt not a multiple of 32
    (2, (1, 300, 20), (2, 310, 25)),        # the production two-chunk split
    (1, (2, 12, 2), (5, 14, 4)),            # Zt = 2: a workgroup holds 24 voxels
    (2, (3, 20, 44), (5, 22, 46)),
    (1, (2, 16, 64), (3, 18, 70)),
    (2, (1, 40, 256), (2, 42, 258)),        # rows clamp at depth: two chunks of 20
    (64, (2, 4, 6), (7, 9, 11)),            # kStemMaxB: 64 distinct origins, every slot of the by-value arrays
]


def _check_stem_sample(b, framed16, w, bias, aff, outs, rows, label):
    """All four apply modes and both partial sets of tile b against float64 (bounds: test_stem_apply_modes_vs_float64),
    in slabs of x planes (a stem workgroup never spans two planes)."""
    Xt, Yt, Zt = (s - 2 for s in framed16.shape)
    nyc = -(-Yt // rows)
    ntile = -(-rows * Zt // 32)
    depth = -(-ntile // 4) + 10        # per lane ceil(ntile / 4) sequential adds of a 2-deep pairwise sum, 5 shuffles, 3 waves
    slab = max(1, 200_000 // (Yt * Zt))
    for x0 in range(0, Xt, slab):
        x1 = min(Xt, x0 + slab)
        sl = {m: outs[m][b, x0:x1] for m in (1, 2, 3, 4)}
        sl["p0"], sl["p2"] = (outs[k][b, x0 * nyc:x1 * nyc] for k in ("p0", "p2"))
        _check_stem_slab(framed16[x0:x1 + 2], w, bias, aff, sl, rows, depth, f"{label} tile {b} x {x0}..{x1}")


def _check_stem_slab(framed16, w, bias, aff, outs, rows, depth, label):
    a64, c64 = aff[0].double(), aff[1].double()
    P = _patches(framed16.double())                                 # (x, Yt, Zt, 27)
    w27 = _tap_major(w).double()
    dw, _ = _split_err(w27)
    y = P @ w27 + bias.double()
    S = P.abs() @ w27.abs() + bias.double().abs()
    e_y = P.abs() @ dw + 57 * U * S                                 # split residue + 55 terms accumulated in fp32
    del P
    t = a64 * y + c64
    e_t = a64.abs() * e_y * (1 + U) + U * t.abs()                   # fmaf: one rounding
    assert t.abs().max() < 80, "the silu bound assumes __expf stays finite"
    z = F.silu(t)
    E_r = 1.1 * e_t + z.abs() * (t.abs() + e_t + 8) * U             # __expf, add, rcpf, product
    # MODE 1: fp16 store
    o1 = outs[1].double()
    _within((o1 - z).abs(), E_r + 0.5 * _ulp16(z.abs() + E_r), "stem MODE 1", f"{label}: MODE 1")
    # MODE 3: split pair
    hi3, lo3 = outs[3][..., :32], outs[3][..., 32:]
    v3 = hi3.double() + lo3.double()
    err3 = (v3 - z).abs()
    b3 = E_r + 2.0 ** -22 * (z.abs() + E_r) + 2.0 ** -25
    _within(err3, b3, "stem MODE 3", f"{label}: MODE 3")
    # MODE 4: hi halves = MODE 3's, x8 = e4m3(16 x), lo8 = e4m3(2^15 (x - hi)), RNE, saturating
    o4 = outs[4]
    assert torch.equal(o4[..., :32].view(torch.int16), hi3.view(torch.int16)), f"{label}: MODE 4 hi halves"
    tail = o4[..., 32:].contiguous().view(torch.uint8)
    x8 = tail[..., :32].contiguous().view(torch.float8_e4m3fn).double()
    lo8 = tail[..., 32:].contiguous().view(torch.float8_e4m3fn).double()
    assert not torch.isnan(x8).any() and not torch.isnan(lo8).any()
    want8 = (16 * v3).clamp(-448, 448)
    d8 = 16 * b3                                                    # v3 is x to b3
    _within((x8 - want8).abs(), (want8.abs() + d8) / 16 + 2.0 ** -10 + d8, "stem MODE 4 x8", f"{label}: x8")
    wantl = (32768 * lo3.double()).clamp(-448, 448)
    dl = 32768 * (0.5 * _ulp16(lo3.double()) + 2.0 ** -25)         # lo3 is x - hi to half its own fp16 ulp
    _within((lo8 - wantl).abs(), (wantl.abs() + dl) / 16 + 2.0 ** -10 + dl, "stem MODE 4 lo8", f"{label}: lo8")
    sat = (16 * z).abs() > 448 + 16 * E_r
    assert (x8[sat].abs() == 448).all(), f"{label}: x8 saturation"
    # MODE 2: raw fp16 store
    r2 = outs[2].double()
    _within((r2 - y).abs(), e_y + 0.5 * _ulp16(y.abs() + e_y), "stem MODE 2", f"{label}: MODE 2")
    # partials
    s_want, sq_want = _block_sums(y, rows), _block_sums(y * y, rows)
    s_bnd = (depth + 1) * U * _block_sums(y.abs(), rows) + _block_sums(e_y, rows)
    sq_bnd = (depth + 2) * U * _block_sums(y * y, rows) + _block_sums(2 * y.abs() * e_y + e_y * e_y, rows)
    for name in ("p0", "p2"):
        p = outs[name].double()
        _within((p[..., 0] - s_want).abs(), s_bnd, "stem partial sums", f"{label}: {name} sums")
        _within((p[..., 1] - sq_want).abs(), sq_bnd, "stem partial sums of squares", f"{label}: {name} sums of squares")
    return bool(sat.any())


def _run_stem_case(ffi, vol, origins, tile, seed, label):
    B = len(origins)
    Xt, Yt, Zt = tile
    w, bias, gamma, beta = _stem_weights(seed)
    mean, std = 127.3, 73.91
    wt, bd = _tap_major(w).to(DEV), bias.to(DEV)
    vol_d = vol.to(DEV)
    ws, p0 = _stem_stats(ffi, vol_d, origins, tile, mean, std, wt, bd)
    p_fin = p0.clone()
    nblk = p0.shape[1]
    aff = torch.empty((B, 2, 32), device=DEV)
    gd, btd = gamma.to(DEV), beta.to(DEV)
    ffi.check(ffi.lib.sk_groupnorm_finalize(_ptr(p_fin), B, nblk, 8, 32, Xt * Yt * Zt, _ptr(gd), _ptr(btd), 1e-5, _ptr(aff),
                                            _st()))
    torch.cuda.synchronize()
    # samples of a uniform image have near-identical statistics: make the affines differ, and drive sample 1's first
    # four channels past |x| = 28 (x8 = e4m3(16 x) saturates)
    k = torch.arange(B, device=DEV, dtype=torch.float32).view(B, 1)
    aff[:, 0] *= 1 + 0.05 * k
    aff[:, 1] += 0.21 * (k % 5)
    if B > 1:
        aff[1, 0, :4], aff[1, 1, :4] = 2.0, 30.0
    outs = {m: _stem_apply(ffi, m, ws, tile, B, wt, bd, aff).cpu() for m in (1, 3, 4)}
    ws2, p2, raw = _stem_stats(ffi, vol_d, origins, tile, mean, std, wt, bd, raw=True)
    assert torch.equal(ws2, ws)
    outs[2], outs["p0"], outs["p2"] = raw.cpu(), p0.cpu(), p2.cpu()
    framed = ws.cpu()[:B * (Xt + 2) * (Yt + 2) * (Zt + 2)].reshape(B, Xt + 2, Yt + 2, Zt + 2)
    rows = _stem_rows(Yt, Zt)
    affc = aff.cpu()
    for b, o in enumerate(origins):
        want = torch.from_numpy(_norm_rule(vol.numpy(), o, tile, mean, std))
        assert torch.equal(framed[b].view(torch.int16), want.view(torch.int16)), f"{label}: normalisation of tile {b}"
        _check_stem_sample(b, framed[b], w, bias, affc[b], outs, rows, label)


@pytest.mark.parametrize("B,tile,vol_shape", STEM_CASES)
def test_stem_apply_modes_vs_float64(ffi, B, tile, vol_shape):
    """sk_conv3d_stem -> sk_groupnorm_finalize -> sk_conv3d_stem_apply / _split / _mix8, and sk_conv3d_stem_raw, on a uint8
    image with the random-init stem weights, against y64 = conv64(norm16, w) + b and z64 = silu(a_b y64 + c_b) with the
    affine the kernels were given (per sample; they differ, and one sample saturates the fp8 x8 code).  Bounds per voxel:
      e_y = sum |x| |w - hi - lo| + 57 u (|b| + sum |x| |w|)        (raw conv: exact products, 55 fp32-accumulated terms)
      E_r = 1.1 (|a| e_y + u |a y + c|) + |z| (|t| + e_t + 8) u     (fmaf, then __expf / add / rcpf / product)
      MODE 1: E_r + ulp16 / 2;  MODE 3: E_r + 2^-22 |z| + 2^-25;  MODE 2 against y64: e_y + ulp16 / 2;
      MODE 4: hi bit-equal to MODE 3's; x8, lo8 within half an e4m3 ulp (2^-4 relative, 2^-10 subnormal) of the codes of
      16 (hi + lo) and 2^15 lo, plus what the MODE 3 pair leaves unknown;
      partials: (depth + 1) u sum |y| + sum e_y, depth = ceil(ceil(rows Zt / 32) / 4) + 10 sequential fp32 additions."""
    g = torch.Generator().manual_seed(sum(vol_shape) + B)
    vol = torch.randint(0, 256, vol_shape, generator=g).to(torch.float16)
    origins = _stem_case_origins(vol_shape, tile, B, B * 7 + tile[1])
    assert len(set(origins)) == B
    _run_stem_case(ffi, vol, origins, tile, 5 + B, f"{B}x{tile}")


def test_stem_apply_modes_production_tile(ffi):
    """The production launch: 300 x 300 x 20 tiles (two y chunks of 150 rows, 600 workgroups per tile) of a
    1024 x 1024 x 256 volume at origins (0, 0, 0) and (724, 724, 236), every voxel of both tiles in float64 (bounds as in
    test_stem_apply_modes_vs_float64)."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    g = torch.Generator(device=DEV).manual_seed(21)
    vol = torch.randint(0, 256, (1024, 1024, 256), generator=g, device=DEV, dtype=torch.uint8).to(torch.float16).cpu()
    _run_stem_case(ffi, vol, [(0, 0, 0), (724, 724, 236)], (300, 300, 20), 3, "production")


# ============================================================================================ heads
def _heads_weights(seed):
    """Random-init heads (unet.random_state_dict's recipe) with five clearly different biases."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.rand((5, 32), generator=g) * 2 - 1) / 32 ** 0.5
    b = torch.tensor([0.31, -0.17, 0.05, -1.3, 1.9])
    return W, b


def _run_heads(ffi, x, aff, W, b, tile, split=False, box=None, prefill=SENT):
    B = x.shape[0]
    X, Y, Z = tile
    out = torch.full((B, 5, X, Y, Z), prefill, dtype=torch.float16, device=DEV)
    i3 = C.c_int32 * 3
    lo = i3(*box[0]) if box is not None else None
    hi = i3(*box[1]) if box is not None else None
    fn = ffi.lib.sk_heads_split if split else ffi.lib.sk_heads
    Wd, bd = W.to(DEV), b.to(DEV)
    ffi.check(fn(_ptr(x), _ptr(aff), _ptr(Wd), _ptr(bd), _ptr(out), B, X, Y, Z, 32, lo, hi, _st()))
    torch.cuda.synchronize()
    return out


def _act_check(out, L, e_L, label):
    """out (B, 5, n) fp16 against tanh / sigmoid of the float64 logits L (B, n, 5) known to e_L (module docstring:
    the tanh form 1 - 2 rcpf(1 + __expf(2 L)) is off by (4 |L| + 11) u absolute, sigmoid by s (|L| + 5) u)."""
    L, e_L = L.transpose(1, 2), e_L.transpose(1, 2)
    got = out.reshape(L.shape).double()
    th, sg = torch.tanh(L[:, :3]), torch.sigmoid(L[:, 3:])
    e_th = e_L[:, :3] + (4 * L[:, :3].abs() + 11) * U
    e_sg = e_L[:, 3:] / 4 + sg * (L[:, 3:].abs() + 5) * U
    want = torch.cat([th, sg], dim=1)
    e = torch.cat([e_th, e_sg], dim=1)
    bnd = e + 0.5 * _ulp16(want.abs() + e)
    err = (got - want).abs()
    _within(err, bnd, label, f"{label} (worst channel {int(((err / bnd).amax(dim=(0, 2))).argmax())})")


def _silu_err(t, e_t):
    return 1.1 * e_t + F.silu(t).abs() * (t.abs() + e_t + 8) * U


HEAD_TILES = [(3, 5, 7), (4, 9, 20)]


@pytest.mark.parametrize("tile", HEAD_TILES)
@pytest.mark.parametrize("with_affine", [False, True])
def test_heads_vs_float64(ffi, tile, with_affine):
    """sk_heads, activated input (affine NULL) and raw input with the affine applied on load (B = 3, different affines):
    reference z = fp16(silu(a x + c)) (or x), logits in float64, tanh on channels 0-2, sigmoid on 3-4.  Bound: the fp16
    store, plus sum_c |W_kc| (ulp16(z_c) + E_r) for the activation's own rounding, plus the logits' fp32 accumulation
    (sum |z| |W - hi - lo| + 65 u (|b| + sum |z||W|)), plus the fp32 tanh / sigmoid (see _act_check)."""
    g = torch.Generator().manual_seed(sum(tile) + with_affine)
    B, n = 3, tile[0] * tile[1] * tile[2]
    W, b = _heads_weights(4)
    x = (torch.randn((B, n, 32), generator=g) * 1.5).half()
    aff = None
    if with_affine:
        aff = torch.stack([torch.rand((B, 32), generator=g) + 0.5, torch.randn((B, 32), generator=g) * 0.5], dim=1)
        aff[1, 0] *= 3.0
        aff[2, 1] -= 1.0
        t = aff[:, 0:1].double() * x.double() + aff[:, 1:2].double()
        z64 = F.silu(t)
        zr = z64.half().double()
        dz = _ulp16(z64.abs() + _silu_err(t, U * t.abs())) + _silu_err(t, U * t.abs())
    else:
        zr, dz = x.double(), torch.zeros((B, n, 32), dtype=torch.float64)
    out = _run_heads(ffi, x.to(DEV), None if aff is None else aff.to(DEV), W, b, tile)
    dW, _ = _split_err(W)
    W64 = W.double()
    L = zr @ W64.t() + b.double()
    S = zr.abs() @ W64.abs().t() + dz @ W64.abs().t() + b.double().abs()
    e_L = dz @ W64.abs().t() + zr.abs() @ dW.t() + 65 * U * S
    _act_check(out.cpu(), L, e_L, f"sk_heads affine={with_affine}")


def test_heads_exact_integer_logits(ffi):
    """Integer z, W and bias, affine NULL: every product and sum is an exact integer in fp32, so each output is
    tanh / sigmoid of a KNOWN integer to half an fp16 ulp plus the fp32 evaluation of the activation.  Pins the
    channel -> row mapping, row 4 (the upper half-wave's register 0) included: the five biases differ by integers."""
    g = torch.Generator().manual_seed(3)
    B, tile = 2, (5, 7, 9)
    n = tile[0] * tile[1] * tile[2]
    z = torch.randint(-1, 2, (B, n, 32), generator=g).half()
    W = torch.randint(-1, 2, (5, 32), generator=g).float()
    W[:, :4] = 0.0
    b = torch.tensor([-3.0, 1.0, 2.0, -2.0, 3.0])
    for k in range(5):
        W[k, k] = 1.0      # each row reads its own channel plus the common random tail
    out = _run_heads(ffi, z.to(DEV), None, W, b, tile)
    L = z.double() @ W.double().t() + b.double()
    _act_check(out.cpu(), L, torch.zeros_like(L), "integer logits")
    for split in (False, True):   # the split form on an exact pair (lo = 0) gives the same answer
        zs = torch.cat([z, torch.zeros_like(z)], dim=-1)
        o = _run_heads(ffi, zs.to(DEV), None, W, b, tile, split=True) if split else out
        assert torch.equal(o, out)


@pytest.mark.parametrize("with_affine", [False, True])
def test_heads_split_vs_float64(ffi, with_affine):
    """sk_heads_split, activated pair (affine NULL: x = hi + lo exactly) and raw pair with the affine applied on load, against
    float64 logits of x (or of z64 = silu(a x + c)).  The kernel re-splits the fp32 activation into raw + bl and multiplies
    w_hi (raw + bl) + w_lo raw: the dropped w_lo bl term is computed exactly where bl is known (affine NULL) and bounded by
    |w_lo| ulp16(z) / 2 otherwise; 97 fp32-accumulated terms."""
    from skoots_amd import unet
    g = torch.Generator().manual_seed(17 + with_affine)
    B, tile = 3, (4, 9, 20)
    n = tile[0] * tile[1] * tile[2]
    W, b = _heads_weights(6)
    xf = torch.randn((B, n, 32), generator=g) * 1.5
    pair = unet.split_pair(xf)
    v = unet.join_pair(pair).double()                          # exactly hi + lo (22 bits fit in fp32)
    dW, W_lo = _split_err(W)
    W64 = W.double()
    aff = None
    if with_affine:
        aff = torch.stack([torch.rand((B, 32), generator=g) + 0.5, torch.randn((B, 32), generator=g) * 0.5], dim=1)
        aff[1, 0] *= 3.0
        t = aff[:, 0:1].double() * v + aff[:, 1:2].double()
        z = F.silu(t)
        E_r = _silu_err(t, U * t.abs())
        dz = E_r + 2.0 ** -22 * (z.abs() + E_r) + 2.0 ** -25
        dropped = (0.5 * _ulp16(z.abs() + E_r)) @ W_lo.abs().t()
    else:
        z, dz = v, torch.zeros_like(v)
        v32 = unet.join_pair(pair)
        raw = v32.half()
        bl = (v32 - raw.float()).half().double()
        dropped = bl.abs() @ W_lo.abs().t()
    out = _run_heads(ffi, pair.to(DEV), None if aff is None else aff.to(DEV), W, b, tile, split=True)
    L = z @ W64.t() + b.double()
    S = (z.abs() + dz) @ W64.abs().t() * (1 + 2.0 ** -10) + b.double().abs()
    e_L = dz @ W64.abs().t() + z.abs() @ dW.t() + dropped + 97 * U * S
    _act_check(out.cpu(), L, e_L, f"sk_heads_split affine={with_affine}")


@pytest.mark.parametrize("tile", [(4, 9, 20), (3, 5, 7), (37, 14, 20)])
def test_heads_fused_activation_equals_separate_pass(ffi, tile):
    """sk_heads(raw, affine) == sk_heads(sk_groupnorm_silu(raw, affine), NULL) BIT FOR BIT: the on-load activation is
    sk_groupnorm_silu's arithmetic op for op (sk::round_t16 in both).  The same for the split form against
    sk_groupnorm_silu_split: fused, the fp32 activation r is split into fp16(r) + fp16(r - fp16(r)); unfused, the stored
    pair (rh, rl) is re-split, fp16(rh + rl) -- which is rh unless rl is exactly half an ulp of an odd rh (then the
    round-to-even moves it; rl is often an fp16 subnormal, so this happens on a few % of the voxels): only such voxels
    may differ, and by at most one fp16 ulp of the output."""
    from skoots_amd import unet
    g = torch.Generator().manual_seed(tile[0] * 13 + tile[2])
    B = 3
    n = tile[0] * tile[1] * tile[2]
    W, b = _heads_weights(8)
    aff = torch.stack([torch.rand((B, 32), generator=g) + 0.5, torch.randn((B, 32), generator=g) * 0.5], dim=1).to(DEV)
    aff[2, 0] *= 2.0
    x = (torch.randn((B, n, 32), generator=g) * 2).half().to(DEV)
    fused = _run_heads(ffi, x, aff, W, b, tile)
    act = x.clone()
    ffi.check(ffi.lib.sk_groupnorm_silu(_ptr(act), _ptr(aff), B, n, 32, _st()))
    plain = _run_heads(ffi, act, None, W, b, tile)
    assert torch.equal(fused, plain)
    xs = unet.split_pair(torch.randn((B, n, 32), generator=g) * 2).to(DEV)
    fused_s = _run_heads(ffi, xs, aff, W, b, tile, split=True)
    act_s = xs.clone()
    ffi.check(ffi.lib.sk_groupnorm_silu_split(_ptr(act_s), _ptr(aff), B, n, 32, _st()))
    plain_s = _run_heads(ffi, act_s, None, W, b, tile, split=True)
    torch.cuda.synchronize()
    rh, rl = act_s[..., :32].cpu(), act_s[..., 32:].cpu()
    moved = ((rh.float() + rl.float()).half() != rh).any(dim=-1)          # (B, n): voxels whose pair re-splits differently
    same = (fused_s == plain_s).cpu().all(dim=1).reshape(B, n)
    assert bool(same[~moved].all()), f"{int((~same & ~moved).sum())} voxels differ"
    # where the re-split moved, the logits differ by |w_lo| ulp16(rh) (~2^-22 relative): at most one fp16 ulp apart
    steps = (fused_s.view(torch.int16).int() - plain_s.view(torch.int16).int()).abs().cpu()
    moved_steps = steps.amax(dim=1).reshape(B, n)[moved]
    assert moved_steps.numel() == 0 or int(moved_steps.max()) <= 1


def _prod_box():
    from tests.test_hip_geometry import TILE, _box
    lo, hi = _box()
    return TILE, (tuple(lo), tuple(hi))


HEAD_BOXES = [   # (tile, box): full tile, ragged interior (nbox % 32 != 0), one voxel, one x plane, boxes on each face
    ((9, 12, 20), ((0, 0, 0), (9, 12, 20))),
    ((9, 12, 20), ((2, 3, 1), (7, 10, 18))),
    ((9, 12, 20), ((4, 5, 6), (5, 6, 7))),
    ((9, 12, 20), ((3, 0, 0), (4, 12, 20))),
    ((9, 12, 20), ((0, 2, 3), (2, 11, 17))),
    ((9, 12, 20), ((6, 0, 5), (9, 4, 20))),
    ((9, 12, 20), ((1, 9, 0), (8, 12, 1))),
    ("production", None),
]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("tile,box", HEAD_BOXES)
def test_heads_box(ffi, tile, box, split):
    """A box of every tile: inside it the output equals the unboxed launch bit for bit, outside it every voxel still holds
    the sentinel prefill.  B = 3 with a different affine per sample; the production box of a 300 x 300 x 20 tile
    (test_hip_geometry._box) included."""
    if tile == "production":
        tile, box = _prod_box()
    g = torch.Generator(device=DEV).manual_seed(sum(box[0]) + 3 * sum(box[1]))
    B = 3
    X, Y, Z = tile
    n = X * Y * Z
    W, b = _heads_weights(10)
    aff = torch.stack([torch.rand((B, 32), generator=g, device=DEV) + 0.5, torch.randn((B, 32), generator=g, device=DEV) * 0.5],
                      dim=1).contiguous()
    aff[1, 0] *= 2.0
    x = (torch.randn((B, n, 32 * (2 if split else 1)), generator=g, device=DEV) * 2).half()
    full = _run_heads(ffi, x, aff, W, b, tile, split=split)
    got = _run_heads(ffi, x, aff, W, b, tile, split=split, box=box)
    (x0, y0, z0), (x1, y1, z1) = box
    assert torch.equal(got[..., x0:x1, y0:y1, z0:z1], full[..., x0:x1, y0:y1, z0:z1])
    outside = torch.ones(tile, dtype=torch.bool, device=DEV)
    outside[x0:x1, y0:y1, z0:z1] = False
    assert bool((got[..., outside] == SENT).all())
    assert not bool((full == SENT).any())


# ------------------------------------------------------------------------------------- training heads
NVOX = [1, 63, 8191, 8193, 3 * 8192 + 5, 300_000, 1_100_003]   # last partial block (8192 per block); > 4096 * 256: grid stride


@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("nvox", NVOX)
def test_train_heads_vs_float64(ffi, nvox, twin):
    """sk_train_heads_fwd_f16: logits = z W^T + b, 8 sequential fmaf per lane, two shuffle sums, the bias: 12 u (|b| +
    sum |z||W|).  sk_train_heads_wgrad_f16: dW = dl^T z, db = sum dl per block of 8192 voxels as ceil(min(nvox, 8192) / 64)
    sequential fmaf per lane plus 64 sequential LDS sums, then a float64 sum over blocks rounded once: (depth + 2) u
    sum |dl||z|.  Both builds (the bf16 twin reads bf16 z)."""
    sfx = "_bf16" if twin else ""
    dt = torch.bfloat16 if twin else torch.float16
    L = lambda name: getattr(ffi.lib, name + sfx)
    g = torch.Generator().manual_seed(nvox + twin)
    z = torch.randn((nvox, 32), generator=g).to(dt)
    W = torch.randn((5, 32), generator=g) / 32 ** 0.5
    b = torch.randn(5, generator=g)
    dl = torch.randn((nvox, 5), generator=g)
    zd, Wd, bd, dld = z.to(DEV), W.to(DEV), b.to(DEV), dl.to(DEV)
    logits = torch.full((nvox, 5), SENT, device=DEV)
    ffi.check(L("sk_train_heads_fwd_f16")(_ptr(zd), _ptr(Wd), _ptr(bd), _ptr(logits), nvox, _st()))
    dW = torch.full((5, 32), SENT, device=DEV)
    db = torch.full((5,), SENT, device=DEV)
    ws = torch.empty(int(L("sk_train_heads_wgrad_workspace_floats")(nvox)), device=DEV)
    ffi.check(L("sk_train_heads_wgrad_f16")(_ptr(zd), _ptr(dld), _ptr(dW), _ptr(db), nvox, _ptr(ws), _st()))
    torch.cuda.synchronize()
    z64, W64, b64, dl64 = z.double(), W.double(), b.double(), dl.double()
    want = z64 @ W64.t() + b64
    bnd = 12 * U * (z64.abs() @ W64.abs().t() + b64.abs())
    _within((logits.cpu().double() - want).abs(), bnd, "train heads logits", f"logits nvox={nvox}{sfx}")
    depth = -(-min(nvox, 8192) // 64) + 64
    wW, wb = dl64.t() @ z64, dl64.sum(dim=0)
    _within((dW.cpu().double() - wW).abs(), (depth + 2) * U * (dl64.abs().t() @ z64.abs()), "train heads dW", f"dW nvox={nvox}{sfx}")
    _within((db.cpu().double() - wb).abs(), (depth + 2) * U * dl64.abs().sum(dim=0), "train heads db", f"db nvox={nvox}{sfx}")


# ============================================================================================ D: argument checks
def _guarded(n, dtype, margin):
    """A device buffer of n elements inside a larger allocation with `margin` elements of slack on both sides, all SENT."""
    big = torch.full((n + 2 * margin,), SENT, dtype=dtype, device=DEV)
    return big, big[margin:margin + n]


def _stem_call(ffi, entry, X=16, Y=16, Z=16, origins=((0, 0, 0), (12, 10, 8)), B=None, tile=(4, 6, 8), cout=32):
    """One stem entry point with buffers sized for the VALID call (B <= 65 tiles of up to (4, 6, 8), an image with slack
    around it): returns (rc, [every buffer the call could have written])."""
    B = len(origins) if B is None else B
    Xt, Yt, Zt = tile
    cap_ws = ffi.lib.sk_conv3d_stem_workspace_bytes(max(B, 2), 4, 6, 8) // 2
    cap_ws = max(cap_ws, (Xt + 2) * (Yt + 2) * (Zt + 2) * max(B, 2))
    _, ws = _guarded(cap_ws, torch.float16, 0)
    nblk = max(ffi.lib.sk_conv3d_stem_num_blocks(4, 6, 8), Xt * Yt)
    part = torch.full((max(B, 2) * nblk * 16,), SENT, device=DEV)
    out = torch.full((max(B, 2) * max(Xt * Yt * Zt, 4 * 6 * 8) * 64,), SENT, dtype=torch.float16, device=DEV)
    _, img = _guarded(X * Y * Z, torch.float16, 4 * Y * Z)
    img.zero_()
    w, bias = torch.ones((27, 32), device=DEV), torch.ones(32, device=DEV)
    aff = torch.ones((max(B, 2), 2, 32), device=DEV)
    org = _org(list(origins) + [(0, 0, 0)] * max(0, B - len(origins)))
    st = _st()
    ws_bytes = cap_ws * 2
    if entry == "stem":
        rc = ffi.lib.sk_conv3d_stem(_ptr(img), X, Y, Z, org, B, Xt, Yt, Zt, 0.0, 1.0, _ptr(w), _ptr(bias), cout, _ptr(part),
                                    _ptr(ws), ws_bytes, st)
    elif entry == "stem_raw":
        rc = ffi.lib.sk_conv3d_stem_raw(_ptr(img), X, Y, Z, org, B, Xt, Yt, Zt, 0.0, 1.0, _ptr(w), _ptr(bias), cout, _ptr(out),
                                        _ptr(part), _ptr(ws), ws_bytes, st)
    elif entry == "train_stem":
        imgf = torch.zeros(max(B, 2) * max(Xt * Yt * Zt, 4 * 6 * 8), device=DEV)
        rc = ffi.lib.sk_train_stem_fwd_f16(_ptr(imgf), B, Xt, Yt, Zt, _ptr(w), _ptr(bias), _ptr(out), _ptr(part), _ptr(ws),
                                           ws_bytes, st)
    else:
        fn = {"apply": ffi.lib.sk_conv3d_stem_apply, "apply_split": ffi.lib.sk_conv3d_stem_apply_split,
              "apply_mix8": ffi.lib.sk_conv3d_stem_apply_mix8}[entry]
        rc = fn(B, Xt, Yt, Zt, _ptr(w), _ptr(bias), _ptr(aff), _ptr(out), cout, _ptr(ws), st)
    torch.cuda.synchronize()
    return rc, [ws, part, out]


STEM_ENTRIES = ["stem", "stem_raw", "apply", "apply_split", "apply_mix8"]
STEM_REFUSALS = [   # (name, kwargs of _stem_call, entry points it applies to)
    ("odd_Zt", dict(tile=(4, 6, 7)), STEM_ENTRIES + ["train_stem"]),
    ("B_65", dict(origins=[(0, 0, 0)] * 65), STEM_ENTRIES + ["train_stem"]),
    ("cout_16", dict(cout=16), STEM_ENTRIES),
    ("overhang_4", dict(origins=((0, 0, 0), (12, 10, 12))), ["stem", "stem_raw"]),
    ("negative_origin", dict(origins=((0, 0, 0), (0, -1, 0))), ["stem", "stem_raw"]),
    ("Zt_0", dict(tile=(4, 6, 0)), STEM_ENTRIES + ["train_stem"]),
    ("Xt_0", dict(tile=(0, 6, 8)), STEM_ENTRIES + ["train_stem"]),
    ("Yt_negative", dict(tile=(4, -6, 8)), STEM_ENTRIES + ["train_stem"]),
    ("lds_too_deep", dict(tile=(1, 1, 4000), Z=4000, origins=((0, 0, 0),)), STEM_ENTRIES + ["train_stem"]),
]


@pytest.mark.parametrize("name,kw,entries", STEM_REFUSALS, ids=[r[0] for r in STEM_REFUSALS])
def test_stem_refuses_bad_arguments_before_any_launch(ffi, name, kw, entries):
    """Odd Zt, B = 65 > kStemMaxB, cout != 32, an overhang of 4, a negative origin, empty extents and a tile depth whose
    staged planes exceed 60 KiB of LDS raise ValueError (SK_ERR_ARG) on every stem entry point they apply to, and the
    workspace, partial and output buffers (real device buffers sized for a valid call) still hold their sentinel fill:
    a refused call has launched nothing."""
    for entry in entries:
        rc, bufs = _stem_call(ffi, entry, **kw)
        with pytest.raises(ValueError):
            ffi.check(rc)
        for t in bufs:
            assert bool((t == SENT).all()), f"{entry}: a refused call wrote a buffer"


HEAD_REFUSALS = [   # (name, (lo, hi) box or None, C)
    ("empty_box", ((2, 2, 2), (2, 5, 6)), 32),
    ("box_past_x", ((0, 0, 0), (6, 5, 6)), 32),
    ("box_past_z", ((1, 1, 1), (3, 4, 7)), 32),
    ("box_negative", ((0, -1, 0), (3, 4, 5)), 32),
    ("C_64", None, 64),
    ("C_16", None, 16),
]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name,box,Cin", HEAD_REFUSALS, ids=[r[0] for r in HEAD_REFUSALS])
def test_heads_refuse_bad_arguments(ffi, name, box, Cin, split):
    """An empty box, a box reaching outside the tile and C != 32 raise ValueError on sk_heads and sk_heads_split; the
    output (with slack around it, so a missed check could not write outside the allocation) keeps its sentinel fill."""
    B, tile = 2, (5, 5, 6)
    n = tile[0] * tile[1] * tile[2]
    margin = 5 * tile[1] * tile[2] * 2
    big, out = _guarded(B * 5 * n, torch.float16, margin)
    _, x = _guarded(B * n * 64 * 2, torch.float16, 64 * tile[1] * tile[2] * 2)
    x.zero_()
    W, b = torch.ones((5, 64), device=DEV), torch.ones(5, device=DEV)
    i3 = C.c_int32 * 3
    lo, hi = (i3(*box[0]), i3(*box[1])) if box is not None else (None, None)
    fn = ffi.lib.sk_heads_split if split else ffi.lib.sk_heads
    rc = fn(_ptr(x), None, _ptr(W), _ptr(b), _ptr(out), B, *tile, Cin, lo, hi, _st())
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ffi.check(rc)
    assert bool((big == SENT).all())
