// Patch geometry and LDS-DMA bookkeeping of conv3_px_kernel and conv3_pxm_kernel, included inside both kernel bodies (text
// inclusion, not a function: see conv3_px_steps.inc).  Takes a, patch, w, lane, c16, g, NPOSP and kLineBytes (bytes per
// voxel line of the source) from the including kernel.
// ---- patch geometry (conv3_m16_kernel's, one column tile per wave) ---------------------------
const int pitch = a.pitch;
int off, ybase, zbase, q_row, out_vox0, tile_nvox;
int svy, svz;             // (y, z) of the voxel this lane STORES: column c16 + 16 (g & 1) of the wave's tile
unsigned vflags = 0;      // bit j: voxel 16 j + c16 on the z = 0 face | << 8: on the z = Zt-1 face | << 16: inside the tile
auto zlo = [&](int j) { return (vflags >> j) & 1u; };
auto zhi = [&](int j) { return (vflags >> (8 + j)) & 1u; };
auto vvalid = [&](int j) { return (vflags >> (16 + j)) & 1u; };
// linear mode only (Zt <= 40, conv3_m16_kernel's comment): region position q <-> in-plane voxel v0 - Zt - 1 + q
const int needed = kPatch + 2 * a.Zt + 2;   // positions a plane really holds; NPOSP rounds it up to a DMA granule
{
    const int v0 = patch * kPatch;
    off = v0 - a.Zt - 1;
    ybase = 0;
    zbase = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int v = v0 + 32 * w + 16 * j + c16;
        const int vy = v / a.Zt, vz = v - vy * a.Zt;
        vflags |= (unsigned)(v < a.Yt * a.Zt) << (16 + j);
        vflags |= (unsigned)(vz == 0) << j;
        vflags |= (unsigned)(vz == a.Zt - 1) << (8 + j);
        if (j == 0) q_row = v - off;
    }
    out_vox0 = v0 + 32 * w;
    tile_nvox = a.Yt * a.Zt;
    const int sv = out_vox0 + c16 + 16 * (g & 1);
    svy = sv / a.Zt;
    svz = sv - svy * a.Zt;
}
const bool sbox = !a.has_box || (svy >= a.box_lo[1] && svy < a.box_hi[1] && svz >= a.box_lo[2] && svz < a.box_hi[2]);

// ---- LDS-DMA bookkeeping: this lane's slots of a plane (conv3_m16_kernel's swizzle) -----------
constexpr int ndma = NPOSP / 16;
int d_vox[kMaxDma];
const int d_cs = ((lane & 3) ^ (((lane >> 4) & 1) << 1)) * 16;
#pragma unroll
for (int k = 0; k < kMaxDma; ++k) {
    const int t = w + 4 * k;
    const int q = (64 * t + lane) >> 2;
    const int Pq = q + off;
    const int y = ybase + (Pq >= 0 ? Pq / pitch : -1), z = zbase + (Pq >= 0 ? Pq % pitch : 0);
    // positions >= needed are padding that the LDS-DMA never writes (d_vox -2: the lane sits out of the instruction):
    // two of them hold the bias / the GroupNorm coefficients of a raw source, the last four are the zero window
    const bool ok = (t < ndma) && y >= 0 && y < a.Yt && z >= 0 && z < a.Zt;
    d_vox[k] = q >= needed ? -2 : (ok ? (y * a.Zt + z) * kLineBytes + d_cs : -1);   // the BYTE offset of this lane's 16-byte piece in a plane of kLineBytes voxel lines
}
