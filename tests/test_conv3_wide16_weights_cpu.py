"""The A fragments of conv3_m16_kernel<64 | 128, XS> (skoots_amd/csrc/conv3d.hip, the wide form on v_mfma_f32_16x16x32_f16) are
read out of the weight image that sk_conv3d_pack_weight_host lays out for conv3_kernel's v_mfma_f32_32x32x16_f16:
[chunk32][dy*3+dz][ks(2)][dx][nt] fragments of 1 KiB, old lane 32 h + r holding the 8 halves K = 16 ks + 8 h .. of row r.  No
second packing exists; this file restates the kernel's lane -> byte map in Python and applies it to the host image (no GPU).

Lane l = (c16 = l & 15, g = l >> 4) of fragment (chunk, dy*3+dz, dx, cout tile nt, cout half i) loads the 16 bytes at

    ((chunk*9 + dy*3+dz)*2*3*NT + dx*NT + nt)*1024            the ks = 0 fragment of the tap (wave-uniform)
    + (g >> 1)*3*NT*1024 + (32*(g & 1) + c16)*16              per lane: old fragment ks = g >> 1, old lane 32 (g & 1) + 16 i + c16
    + i*256

and they must be fp16(W[32 nt + 16 i + c16][32 chunk + 8 g + j][dx][dy][dz]), j = 0 .. 7: row c16 of the 16 x 32 A operand, K
group g.
"""
import ctypes as C

import numpy as np
import pytest
import torch


def _host_image(w, cout, cin):
    from skoots_amd import _ffi
    fpt = w.numpy().ctypes.data_as(C.POINTER(C.c_float))
    n = _ffi.lib.sk_conv3d_pack_weight_host(fpt, cout, cin, 3, None)
    buf = np.empty(n, dtype=np.uint8)
    assert _ffi.lib.sk_conv3d_pack_weight_host(fpt, cout, cin, 3, buf.ctypes.data_as(C.c_void_p)) == n
    return buf


@pytest.mark.parametrize("cout,cin", [(64, 64), (64, 128), (128, 128)])
def test_wide16_fragments_from_the_32x32x16_image(cout, cin):
    """For every (chunk, tap, nt, i, lane, j) the half gathered by the kernel's address arithmetic equals
    fp16(W[32 nt + 16 i + (l & 15)][32 chunk + 8 (l >> 4) + j][tap]) bit for bit, the gathered bytes stay inside the image, and
    over all fragments every byte of the image is read exactly once (the map is a permutation of the image: nothing is
    read twice, nothing is left out)."""
    gen = torch.Generator().manual_seed(1000 * cout + cin)
    w = torch.randn((cout, cin, 3, 3, 3), generator=gen).contiguous()          # torch layout (co, ci, dx, dy, dz)
    img = _host_image(w, cout, cin)
    NT, nch = cout // 32, cin // 32
    assert img.size == nch * 9 * 2 * 3 * NT * 1024
    halves = torch.from_numpy(img.copy()).view(torch.float16)
    w16 = w.half()
    lane = torch.arange(64)
    c16, g = lane & 15, lane >> 4
    lane_off = (g >> 1) * 3 * NT * 1024 + (32 * (g & 1) + c16) * 16        # bytes
    seen = torch.zeros(img.size // 2, dtype=torch.int32)
    j = torch.arange(8)
    for ch in range(nch):
        for dydz in range(9):
            dy, dz = dydz // 3, dydz % 3
            for dx in range(3):
                for nt in range(NT):
                    base = ((ch * 9 + dydz) * 2 * 3 * NT + dx * NT + nt) * 1024
                    for i in range(2):
                        off = base + lane_off + i * 256                          # (64,) byte offsets, 16 bytes each
                        assert int(off.min()) >= 0 and int(off.max()) + 16 <= img.size
                        idx = (off[:, None] // 2) + j[None, :]                   # (64, 8) half indices
                        got = halves[idx]
                        co = 32 * nt + 16 * i + c16
                        ci = (32 * ch + 8 * g)[:, None] + j[None, :]
                        want = w16[co[:, None], ci, dx, dy, dz]
                        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (ch, dydz, dx, nt, i)
                        seen[idx.reshape(-1)] += 1
    assert bool((seen == 1).all()), f"{int((seen != 1).sum())} halves of the image are not read exactly once"
