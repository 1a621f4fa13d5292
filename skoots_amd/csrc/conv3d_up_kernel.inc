// conv3_upf_kernel's body, included twice by conv3d_up.hip: SK_UPF_MIX8 = 0 -> conv3_upf_kernel (fp16 and split precisions),
// SK_UPF_MIX8 = 1 -> conv3_upf_mix8_kernel (precision "mix8").  Two inclusions instead of a template flag because the phase
// loops of the mix8 form are walked in pairs, and any change to the loop structure of the other variants -- an unrolled
// one-trip inner loop, a lambda around the phase body -- changed their generated code (compared instruction by instruction).
// WLDS (one skip chunk only): tap rows 0 and 1 of the skip chunk's weights sit in LDS behind the ring, one copy per
// workgroup, instead of being streamed by each of the four waves (conv3_m16_kernel's WL): 12 of the 54 + 32 weight loads
// per wave and step become LDS reads and the hand-off to the skip phase requests no weights at all.
// SPLIT (precision "split", sk_conv3d_upfold_split): every tensor holds fp16 hi + lo pairs, [hi (C) | lo (C)] per voxel
// line, and every weight is a hi + lo pair; a logical chunk runs as three phases -- (x_hi, w_lo), (x_hi again: no LDS-DMA,
// w_hi), (x_lo, w_hi) -- as in conv3_m16_kernel's split mode, and the fp32 accumulator is stored as hi = fp16(v),
// lo = fp16(v - hi).  The folded weights are split AFTER the fold (the sum is formed in double on the host).
// MIX8 (precision "mix8", sk_conv3d_upfold_mix8; SPLIT output): sources hold [hi fp16 (C) | per chunk x8 (32 B) | lo8 (32 B)]
// lines; a logical chunk runs as two phases -- its hi halves against w_hi on the fp16 instruction, then ONE block-scaled fp8
// product (v_mfma_scale_f32_16x16x128_f8f6f4) over K = 128 = two taps x {w_lo . x8, w . lo8}: tap rows (dy, dz) in pairs for a
// skip chunk (conv3_m16_kernel's), the two tz taps of a ty for an upsampled chunk.  The phase kind is a compile-time value
// (phases are walked in pairs): a run-time branch between bodies that own all accumulators costs copies and spills.
template <int XS, bool WLDS, bool SPLIT>
__global__ void __launch_bounds__(256, 2) SK_UPF_NAME(UpfArgs a) {
    constexpr bool MIX8 = SK_UPF_MIX8;
    static_assert(!MIX8 || (SPLIT && !WLDS), "mix8 writes split pairs and streams its weights");
    constexpr int R = XS + 2;          // fine planes of a step
    constexpr int RL = XS / 2 + 2;     // low-resolution planes of a step
    static_assert(XS == 4, "x parity of an output plane must be a compile-time constant");
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int py = w >> 1, pz = w & 1;   // parity class of this wave's output voxels
    const int c16 = lane & 15, g = lane >> 4;

    int patch, xc, b, block_in_batch, nblk;
    decode_block(xcd_remap(blockIdx.x), a.npatch, a.nxc, patch, xc, b, block_in_batch, nblk);

    const int Zl = a.Zl, Zt = a.Zt;
    const int yl0 = patch * a.K;             // first low-resolution row of this workgroup
    const int nseg = a.K * Zl;               // columns in use (<= 32)

    // per-lane flags of column (j): bit j: the z-1 tap wraps (class pz = 0, zl = 0) | bit 8 + j: the z+1 tap wraps
    // (pz = 1, zl = Zl-1) | bit 16 + j: a real voxel
    unsigned vflags = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = 16 * j + c16;
        const int r = m / Zl, c = m - r * Zl;
        vflags |= (unsigned)(pz == 0 && c == 0) << j;
        vflags |= (unsigned)(pz == 1 && c == Zl - 1) << (8 + j);
        vflags |= (unsigned)(m < nseg && yl0 + r < a.Yl) << (16 + j);
    }
    auto zlo = [&](int j) { return (vflags >> j) & 1u; };
    auto zhi = [&](int j) { return (vflags >> (8 + j)) & 1u; };
    auto vvalid = [&](int j) { return (vflags >> (16 + j)) & 1u; };

    // the voxel this lane STORES (after the permlane transpose it owns 8 channels of column c16 + 16 (g & 1))
    int ovox;      // in-plane fine voxel index, -1: none
    {
        const int m = c16 + 16 * (g & 1);
        const int r = m / Zl, c = m - r * Zl;
        ovox = (m < nseg && yl0 + r < a.Yl) ? (2 * (yl0 + r) + py) * Zt + 2 * c + pz : -1;
    }

    // ---- LDS-DMA bookkeeping ------------------------------------------------------------
    // fine plane: position q = sub * SUBP + 1 + ylr * Zl + zl, sub = 2 (y & 1) + (z & 1), rows ylr = (y >> 1) - (yl0 - (y & 1))
    const int ndma = a.nposp / 16, ndmal = a.nposl / 16;
    const int d_cs = ((lane & 3) ^ (((lane >> 4) & 1) << 1)) * 16;   // source chunk of this lane's slot (conv3_m16_kernel)
    int d_vox[kMaxDma], d_low[kMaxDmaL];
#pragma unroll
    for (int k = 0; k < kMaxDma; ++k) {
        const int t = w + 4 * k;
        const int q = (64 * t + lane) >> 2;
        const int sub = q / a.SUBP, rem = q - sub * a.SUBP - 1;
        const int ylr = rem >= 0 ? rem / Zl : 0, zl = rem - ylr * Zl;
        const int yp = sub >> 1, zp = sub & 1;
        const int y = 2 * (yl0 - yp + ylr) + yp, z = 2 * zl + zp;
        const bool ok = t < ndma && sub < 4 && rem >= 0 && ylr <= a.K && y >= 0 && y < a.Yt;
        d_vox[k] = ok ? y * Zt + z : -1;
    }
    // low-resolution plane: position q = 1 + (yl - (yl0 - 1)) * Zl + zl
#pragma unroll
    for (int k = 0; k < kMaxDmaL; ++k) {
        const int t = w + 4 * k;
        const int q = (64 * t + lane) >> 2;
        const int rem = q - 1;
        const int ylr = rem >= 0 ? rem / Zl : 0, zl = rem - ylr * Zl;
        const int yl = yl0 - 1 + ylr;
        const bool ok = t < ndmal && rem >= 0 && ylr < a.K + 2 && yl >= 0 && yl < a.Yl;
        d_low[k] = ok ? yl * Zl + zl : -1;
    }

    f32x4 acc[XS][2][2];   // [output plane][cout half i][voxel half j]
    float gsum[2], gsq[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) gsum[q] = gsq[q] = 0.0f;

    const int xa = xc * a.XC;
    const int xb = min(xa + a.XC, a.Xt);
    const int Xl = a.Xt >> 1;
    const int plane_bytes = (a.nposp + sk::kZeroPos) * kPosBytes;
    const int zero_addr = a.nposp * kPosBytes;   // never written by either image's DMA (nposl <= nposp)
    const long long out_plane = (long long)a.Yt * Zt * a.out_vs;
    char* outb = a.out + (long long)b * a.Xt * out_plane;
    const float* biasp = a.bias + a.cout_off + 4 * g;

    const int nsteps = (xb - xa + XS - 1) / XS;
    // Virtual chunks: plain mode one per 32-channel chunk; split mode three -- part 0: hi halves x lo weights, part 1: the
    // SAME staged planes x hi weights (no LDS-DMA), part 2: lo halves x hi weights
    // (mix8: two -- part 0: hi halves x hi weights, part 1: the 8-bit halves x the fp8 weights)
    constexpr int kParts = MIX8 ? 2 : (SPLIT ? 3 : 1);
    constexpr int kLoPart = MIX8 ? 1 : 2;   // the part that stages the second half of the voxel line
    const int nvs = a.ns * kParts, nvu = a.nu * kParts;
    auto v_chunk = [](int v) { return v / kParts; };
    auto v_part = [](int v) { return v % kParts; };
    auto v_dma = [&](int v) { return MIX8 || v_part(v) != 1; };

    // Phase order of a step: the skip chunks, then the upsampled chunks.  Fine plane i of the step lives in ring slot
    // (rot + i) % R; the low-resolution planes of the step take the slots of fine planes 0 .. RL-1, which the step is
    // done with -- fine planes XS, XS + 1 stay staged through the upsampled phases and are planes 0, 1 of the next
    // step's skip chunk when there is only one (`reuse`: XS instead of XS + 2 plane loads per step).
    auto issue_fine = [&](int step, int chs, bool reuse, int rot_n) {
        // the plane offsets of the next step are formed here, not phases earlier: hoisted, they cost the mix8 form 12 spilled
        // registers and the others 14-26 registers and 38 SGPR reloads per step (same-box A/B: -0.8 % fp16, -1.2 % split, -8 % mix8)
        asm volatile("" : "+s"(step));
        const int x0 = xa + step * XS;
        const int xlo = max(x0 - 1, 0);
        const long long wbytes = min((long long)(R + 1) * a.skip_plane, a.skip_batch - (long long)xlo * a.skip_plane);
        const __amdgpu_buffer_rsrc_t rsrc = sk::make_rsrc(a.skip + (long long)b * a.skip_batch + (long long)xlo * a.skip_plane, (unsigned)wbytes);
        const unsigned vstride = (unsigned)(a.skipC * 2 * (SPLIT ? 2 : 1));
        const int choff = v_chunk(chs) * 64 + (v_part(chs) == kLoPart ? a.skipC * 2 : 0);   // split: the lo halves follow the hi halves
        for (int i = reuse ? 2 : 0; i < R; ++i) {
            const int x = x0 - 1 + i;
            const bool xok = x >= 0 && x < a.Xt;
            char* lbase = lds + ((rot_n + i) % R) * plane_bytes;
            const unsigned xoff = (unsigned)((x - xlo) * (int)a.skip_plane + choff + d_cs);
#pragma unroll
            for (int k = 0; k < kMaxDma; ++k) {
                const int t = w + 4 * k;
                if (t < ndma) {
                    int dv = d_vox[k];
                    asm volatile("" : "+v"(dv));   // keep the offset arithmetic here: hoisted out of the step loop it costs registers
                    const unsigned voff = (xok && dv >= 0) ? xoff + (unsigned)dv * vstride : sk::kOob;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lbase + t * 1024), 16, voff, 0, 0, 0);
                }
            }
        }
    };
    auto issue_low = [&](int step, int chu, bool /*reuse: never -- the skip phases overwrite these slots*/, int rotl_n) {
        const int xl0 = ((xa + step * XS) >> 1) - 1;
        const int xlo = max(xl0, 0);
        const long long wbytes = min((long long)(RL + 1) * a.up_plane, a.up_batch - (long long)xlo * a.up_plane);
        const __amdgpu_buffer_rsrc_t rsrc = sk::make_rsrc(a.up + (long long)b * a.up_batch + (long long)xlo * a.up_plane, (unsigned)wbytes);
        const unsigned vstride = (unsigned)(a.upC * 2 * (SPLIT ? 2 : 1));
        const int choff = v_chunk(chu) * 64 + (v_part(chu) == kLoPart ? a.upC * 2 : 0);
        for (int i = 0; i < RL; ++i) {
            const int xl = xl0 + i;
            const bool xok = xl >= 0 && xl < Xl;
            char* lbase = lds + ((rotl_n + i) % R) * plane_bytes;
            const unsigned xoff = (unsigned)((xl - xlo) * (int)a.up_plane + choff + d_cs);
#pragma unroll
            for (int k = 0; k < kMaxDmaL; ++k) {
                const int t = w + 4 * k;
                if (t < ndmal) {
                    const unsigned voff = (xok && d_low[k] >= 0) ? xoff + (unsigned)d_low[k] * vstride : sk::kOob;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lbase + t * 1024), 16, voff, 0, 0, 0);
#if SK_UPF_MIX8
                    // mix8: the small low-resolution planes hold BOTH halves of their lines, the 8-bit halves nposl positions on (the
                    // host checks that they fit a ring slot): the chunk's fp8 phase follows its fp16 phase with no LDS-DMA, wait or
                    // barrier in between (skipping that LDS-DMA in a timing ablation was worth 6 % of dec0.0)
                    const unsigned voff8 = (xok && d_low[k] >= 0) ? voff + (unsigned)(a.upC * 2) : sk::kOob;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lbase + a.nposl * 64 + t * 1024), 16, voff8, 0, 0, 0);
#endif
                }
            }
        }
    };
    const __amdgpu_buffer_rsrc_t wrsrc = sk::make_rsrc(a.wpk, MIX8 ? (unsigned)a.wpk_bytes : (unsigned)((a.ns * kSkipFrags + a.nu * kUpFrags) * (SPLIT ? 2 : 1) * 1024));
    const unsigned wlane = lane * 16;
    auto wload = [&](unsigned off) {
        return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, __builtin_amdgcn_readfirstlane(off), 0));
    };
    // first fragment of a chunk for this wave
    // split: per chunk the lo-weight fragment set, then the hi-weight set; part 0 multiplies by lo, parts 1 and 2 by hi
    // mix8: one fp16 set (w_hi) per chunk, addressed by the chunk of the phase
    auto wbase_skip = [&](int v) {
        return (unsigned)((MIX8 ? v_chunk(v) : (SPLIT ? (2 * v_chunk(v) + (v_part(v) != 0)) : v)) * kSkipFrags * 1024);
    };
    auto wbase_up = [&](int v) {
        const int frag0 = MIX8 ? a.ns * kSkipFrags + v_chunk(v) * kUpFrags
                               : (SPLIT ? 2 * a.ns * kSkipFrags + (2 * v_chunk(v) + (v_part(v) != 0)) * kUpFrags
                                        : a.ns * kSkipFrags + v * kUpFrags);
        return (unsigned)((frag0 + w * 32) * 1024);
    };

    // Weight fragments that cross a phase boundary (requested before the closing barrier of the phase before): ONE
    // register set for both kinds of chunk -- a value carried around the phase loop stays allocated through every phase.
    // skip chunk: wq[ks * 3 + dx] = the two cout halves of a tap row; upsampled chunk: wq[(i*2 + px)*2 + tx]
    // of a (ty, tz) row.
    half8 wq[8];
    auto load_af = [&](unsigned wch, int tytz, half8 (&dst)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[e] = wload(wch + (unsigned)((tytz * 8 + e) * 1024));
    };
    const char* wlds = lds + R * plane_bytes + lane * 16;   // WLDS: fragments 0 .. 11 of the skip chunk
    auto prefetch_skip = [&](int cs) {   // the first fragments of a phase
        if constexpr (WLDS) return;      // row 0 comes from LDS at the start of the phase
#pragma unroll
        for (int e = 0; e < 6; ++e) wq[e] = wload(wbase_skip(cs) + e * 1024);
    };
    half8 wq1[8];   // upsampled chunk: second tap row (live from the hand-off before the phase to its second row only)
    auto prefetch_up = [&](int cu) {
        load_af(wbase_up(cu), 0, wq);
        load_af(wbase_up(cu), 1, wq1);
    };

    if (tid < R * 4 * sk::kZeroPos)
        *reinterpret_cast<uint4*>(lds + (tid / (4 * sk::kZeroPos)) * plane_bytes + zero_addr + (tid % (4 * sk::kZeroPos)) * 16) = make_uint4(0, 0, 0, 0);
    if constexpr (WLDS) {
        for (int i = tid; i < 12 * 64; i += 256)
            *reinterpret_cast<uint4*>(lds + R * plane_bytes + i * 16) = *reinterpret_cast<const uint4*>(a.wpk + i * 16);
    }
    issue_fine(0, 0, false, 0);
    prefetch_skip(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const bool ring = !SPLIT && a.ns == 1;   // the same skip chunk every step: its two trailing planes are reused
    int rot = 0;
    SK_T_DECL
    for (int step = 0; step < nsteps; ++step) {
        const int x0 = xa + step * XS;
#pragma unroll
        for (int o = 0; o < XS; ++o)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[o][i][0] = acc[o][i][1] = *reinterpret_cast<const f32x4*>(biasp + 16 * i);
        // The LDS addresses of the taps are cheap functions of the lane's column: recomputed every step.  Without this
        // opaque copy the compiler hoists all 18 + 8 of them out of the step loop and spills.
        int c16v = c16;
        asm volatile("" : "+v"(c16v));

        // MIX8 walks its phases in (fp16, fp8) pairs with the kind a compile-time value; the other variants keep the plain
        // loop they were tuned with (the loop header is chosen by the preprocessor: their code is unchanged by MIX8's existence)
#if SK_UPF_MIX8
        for (int cs0 = 0; cs0 < nvs; cs0 += 2)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int cs = cs0 + sub;
            const bool f8 = sub == 1;
#else
        for (int cs = 0; cs < nvs; ++cs) {
            constexpr bool f8 = false;
#endif
            const unsigned wch = wbase_skip(cs);
            // ---------------- skip chunk: 27 taps on the de-interleaved fine planes -----------------
            int pslot[R];
#pragma unroll
            for (int i = 0; i < R; ++i) pslot[i] = ((rot + i) % R) * plane_bytes;
            // A body = (tap row, voxel half j): R fragments feeding 6 XS MFMAs (both cout halves); the next body's fragments
            // and the NEXT ROW's six weight fragments are requested before this body's MFMAs.
            half8 bb[2][R];
            half8 wb[6];
            auto load_body = [&](int dydz, int j, half8 (&dst)[R]) {
                const int dy = dydz / 3 - 1, dz = dydz % 3 - 1;
                // fine (y, z) = (2 yl + py + dy, 2 zl + pz + dz): sub-plane by the parities, position offset by the halves
                const int Y = py + dy, Z = pz + dz;
                const int tapoff = ((Y & 1) * 2 + (Z & 1)) * a.SUBP + 1 + (Y >= 1 ? Zl : 0) + (Z >> 1);   // Z >> 1: floor
                const int q = c16v + tapoff;
                int addr = (q * 4 + (g ^ (((q >> 2) & 1) << 1))) * 16 + 1024 * j;   // (q + 16) >> 2 has the parity of q >> 2
                if (dz < 0) addr = zlo(j) ? sk::zero_of(zero_addr, addr) : addr;
                if (dz > 0) addr = zhi(j) ? sk::zero_of(zero_addr, addr) : addr;
#pragma unroll
                for (int i = 0; i < R; ++i) dst[i] = *reinterpret_cast<const half8*>(lds + pslot[i] + addr);
            };
            auto mma_body = [&](int j, const half8* wf, const half8 (&src)[R]) {
#pragma unroll
                for (int i = 0; i < R; ++i)
#pragma unroll
                    for (int d = 0; d < 3; ++d)
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) {
                            const int o = i - d;
                            if (o >= 0 && o < XS) acc[o][ks][j] = SK_MFMA_16x16x32_T16(wf[ks * 3 + d], src[i], acc[o][ks][j], 0, 0, 0);
                        }
            };
            if (f8) {
                if constexpr (MIX8) {
                    typedef int v8i __attribute__((ext_vector_type(8)));
                    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                    // this lane's K block: g >> 1 = which tap row of the pair, g & 1 = x8 (0) | lo8 (1) -- 32 contiguous bytes of the
                    // staged position (two 16-byte slots; the plane swizzle exchanges the 32-byte halves)
                    const int halfsel = (g & 1) * 2;
                    const int sa = a.w8_scale, sb = 0x70707070;   // E8M0: weights 2^-b (host), activations 2^-15
                    const unsigned w8 = (unsigned)a.w8_off + (unsigned)(v_chunk(cs) * kSkipFrags8) * 2048u + wlane * 2;
#pragma unroll 1
                    for (int rp = 0; rp < 5; ++rp) {
                        const int rr = min(2 * rp + (g >> 1), 8);   // (the tenth row does not exist: its weights are zero)
                        const int dz = rr % 3 - 1;
                        const int Y = py + rr / 3 - 1, Z = pz + dz;
                        const int tapoff = ((Y & 1) * 2 + (Z & 1)) * a.SUBP + 1 + (Y >= 1 ? Zl : 0) + (Z >> 1);
                        v8i af[2][3];
#pragma unroll
                        for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
                            for (int d = 0; d < 3; ++d) {
                                const unsigned wo = w8 + (unsigned)(((rp * 2 + i2) * 3 + d) * 2048);
                                const u32x4 w0 = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wo, 0, 0);
                                const u32x4 w1 = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wo + 16, 0, 0);
                                af[i2][d] = v8i{(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], (int)w1[0], (int)w1[1], (int)w1[2], (int)w1[3]};
                            }
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int q = c16v + tapoff;
                            int addr = (q * 4 + (halfsel ^ (((q >> 2) & 1) << 1))) * 16 + 1024 * j;
                            if ((dz < 0 && zlo(j)) || (dz > 0 && zhi(j))) addr = sk::zero_of(zero_addr, addr);
#pragma unroll
                            for (int i = 0; i < R; ++i) {
                                const u32x4 lo4 = *reinterpret_cast<const u32x4*>(lds + pslot[i] + addr);
                                const u32x4 hi4 = *reinterpret_cast<const u32x4*>(lds + pslot[i] + addr + 16);
                                const v8i bf = v8i{(int)lo4[0], (int)lo4[1], (int)lo4[2], (int)lo4[3], (int)hi4[0], (int)hi4[1], (int)hi4[2], (int)hi4[3]};
#pragma unroll
                                for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
                                    for (int d = 0; d < 3; ++d) {
                                        const int o = i - d;
                                        if (o >= 0 && o < XS)
                                            acc[o][i2][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[i2][d], bf, acc[o][i2][j], 0, 0, 0, sa, 0, sb);
                                    }
                            }
                        }
                    }
                }
            } else {
            if constexpr (WLDS) {
#pragma unroll
                for (int e = 0; e < 6; ++e) wq[e] = *reinterpret_cast<const half8*>(wlds + e * 1024);
            }
            load_body(0, 0, bb[0]);
#pragma unroll
            for (int dydz = 0; dydz < 9; ++dydz) {
                half8* wcur = (dydz & 1) ? wb : wq;
                half8* wnext = (dydz & 1) ? wq : wb;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j == 0) {
                        load_body(dydz, 1, bb[1]);
                        if (dydz < 8) {
#pragma unroll
                            for (int e = 0; e < 6; ++e) {
                                if (WLDS && dydz + 1 < 2)
                                    wnext[e] = *reinterpret_cast<const half8*>(wlds + ((dydz + 1) * 6 + e) * 1024);
                                else
                                    wnext[e] = wload(wch + (unsigned)(((dydz + 1) * 6 + e) * 1024));
                            }
                        }
                    } else if (dydz < 8) {
                        load_body(dydz + 1, 0, bb[0]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    mma_body(j, wcur, bb[j]);
                }
            }
            }
            SK_T(0)   // skip MFMA loop
            if (cs + 1 < nvs) {
                // hand the planes to the next skip chunk: barrier (all waves done reading) -> LDS-DMA + first weights of the
                // next phase -> landed -> barrier; split part 1 multiplies the planes that are staged: weights only
                const bool next_f8 = MIX8 && !f8;   // an fp8 phase loads its own fragments
                if (v_dma(cs + 1)) {
                    __syncthreads();
                    issue_fine(step, cs + 1, false, rot);
                    if (!next_f8) prefetch_skip(cs + 1);
                    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
                } else {
                    prefetch_skip(cs + 1);
                }
            }
        }
        // ... and to the first upsampled chunk (outside the loop: the weight rows requested here must not look live
        // through the skip chunks' MFMA loops)
        __syncthreads();
        SK_T(1)   // barrier
        issue_low(step, 0, false, rot);
        prefetch_up(0);
        SK_T(2)   // LDS-DMA issue + weight prefetch
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        SK_T(3)   // landing wait
        asm volatile("s_barrier" ::: "memory");
        SK_T(4)   // barrier

#if SK_UPF_MIX8
        for (int cu0 = 0; cu0 < nvu; cu0 += 2)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int cu = cu0 + sub;
            const bool f8 = sub == 1;
#else
        for (int cu = 0; cu < nvu; ++cu) {
            constexpr bool f8 = false;
#endif
            const unsigned wch = wbase_up(cu);
            // ---------------- upsampled chunk: 2 x 2 x 2 folded taps on the low-resolution planes -----------------
            int pslot[RL];
#pragma unroll
            for (int i = 0; i < RL; ++i) pslot[i] = ((rot + i) % R) * plane_bytes;
            // a body = (tap row (ty, tz), voxel half j): RL fragments feeding 4 XS MFMAs
            half8 bl[2][RL];
#if SK_UPF_MIX8
            int c16u = c16;   // (mix8: the upsampled phases' tap addresses are formed here, not at the top of the step and spilled)
            asm volatile("" : "+v"(c16u));
#else
            const int c16u = c16v;
#endif
            auto load_low = [&](int tytz, int j, half8 (&dst)[RL]) {
                const int sy = (tytz >> 1) + py - 1, sz = (tytz & 1) + pz - 1;   // low-resolution offsets of this tap
                const int q = c16u + 1 + (1 + sy) * Zl + sz;
                int addr = (q * 4 + (g ^ (((q >> 2) & 1) << 1))) * 16 + 1024 * j;
                addr = (sz < 0 && zlo(j)) ? sk::zero_of(zero_addr, addr) : addr;
                addr = (sz > 0 && zhi(j)) ? sk::zero_of(zero_addr, addr) : addr;
#pragma unroll
                for (int i = 0; i < RL; ++i) dst[i] = *reinterpret_cast<const half8*>(lds + pslot[i] + addr);
            };
            // Weight fragments two tap rows ahead: a fragment here feeds 4 MFMAs (2 planes of its x parity x 2 voxel halves)
            // and the four waves stream four different sets, which mostly come from L2 -- one row (32 MFMAs) of lead left
            // the wave waiting on every row (the phase took 5.6x its MFMA cycles).  Rows 0, 1 were requested before the
            // phase's opening barrier (wq, wq1), row 2 goes out now, row 3 takes row 0's registers.
            if (f8) {
                if constexpr (MIX8) {
                    typedef int v8i __attribute__((ext_vector_type(8)));
                    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                    const int halfsel = (g & 1) * 2;
                    const int sa = a.w8_scale, sb = 0x70707070;
                    const unsigned w8 = (unsigned)a.w8_off + (unsigned)(a.ns * kSkipFrags8 + v_chunk(cu) * kUpFrags8 + w * 16) * 2048u + wlane * 2;
                    const int sz = (g >> 1) + pz - 1;   // this lane's K block: the tz tap g >> 1 of the row pair, x8 | lo8 by g & 1
#pragma unroll 1
                    for (int ty = 0; ty < 2; ++ty) {
                        const int sy = ty + py - 1;
                        v8i af[8];   // [(i * 2 + px) * 2 + tx]: the eight fragments of the row pair, once for both voxel halves
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const unsigned wo = w8 + (unsigned)((ty * 8 + e) * 2048);
                            const u32x4 w0 = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wo, 0, 0);
                            const u32x4 w1 = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wo + 16, 0, 0);
                            af[e] = v8i{(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], (int)w1[0], (int)w1[1], (int)w1[2], (int)w1[3]};
                        }
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int q = c16u + 1 + (1 + sy) * Zl + sz;
                            int addr = (q * 4 + (halfsel ^ (((q >> 2) & 1) << 1))) * 16 + 1024 * j + a.nposl * 64;   // the 8-bit halves' image
                            if ((sz < 0 && zlo(j)) || (sz > 0 && zhi(j))) addr = sk::zero_of(zero_addr, addr);
                            v8i bf[RL];
#pragma unroll
                            for (int i = 0; i < RL; ++i) {
                                const u32x4 lo4 = *reinterpret_cast<const u32x4*>(lds + pslot[i] + addr);
                                const u32x4 hi4 = *reinterpret_cast<const u32x4*>(lds + pslot[i] + addr + 16);
                                bf[i] = v8i{(int)lo4[0], (int)lo4[1], (int)lo4[2], (int)lo4[3], (int)hi4[0], (int)hi4[1], (int)hi4[2], (int)hi4[3]};
                            }
#pragma unroll
                            for (int o = 0; o < XS; ++o)
#pragma unroll
                                for (int tx = 0; tx < 2; ++tx)
#pragma unroll
                                    for (int i = 0; i < 2; ++i) {
                                        const int px = o & 1, il = (o >> 1) + tx + px;
                                        acc[o][i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[(i * 2 + px) * 2 + tx], bf[il], acc[o][i][j], 0, 0, 0, sa, 0, sb);
                                    }
                        }
                    }
                }
            } else {
#if SK_UPF_MIX8
            // (mix8: two register sets -- row 2 takes row 0's registers, row 3 row 1's: the third set is what made this kernel
            // spill 46 registers at its phase boundaries, +1.5 GB written and +2.7 GB fetched per 32-tile launch in the PMC passes)
            half8* const wq2 = wq;
#else
            half8 wq2[8];
            load_af(wch, 2, wq2);
#endif
            load_low(0, 0, bl[0]);
#pragma unroll
            for (int tytz = 0; tytz < 4; ++tytz) {
                const half8* af = tytz == 1 ? wq1 : (tytz == 2 ? wq2 : (SK_UPF_MIX8 && tytz == 3 ? wq1 : wq));
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j == 0) {
                        load_low(tytz, 1, bl[1]);
                    } else if (tytz < 3) {
                        load_low(tytz + 1, 0, bl[0]);
                    }
#if SK_UPF_MIX8
                    if (tytz == 1 && j == 0) load_af(wch, 2, wq);    // row 0 is done with wq
                    if (tytz == 2 && j == 0) load_af(wch, 3, wq1);   // row 1 is done with wq1
#else
                    if (tytz == 1 && j == 0) load_af(wch, 3, wq);   // row 0 is done with wq
#endif
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int o = 0; o < XS; ++o)
#pragma unroll
                        for (int tx = 0; tx < 2; ++tx)
#pragma unroll
                            for (int i = 0; i < 2; ++i) {
                                const int px = o & 1, il = (o >> 1) + tx + px;   // low plane of tap tx for output plane o
                                acc[o][i][j] = SK_MFMA_16x16x32_T16(af[(i * 2 + px) * 2 + tx], bl[j][il], acc[o][i][j], 0, 0, 0);
                            }
                }
            }
            }
            const bool last = cu + 1 == nvu;
            const bool have_next = !last || step + 1 < nsteps;
            const int rot_n = (last && ring) ? (rot + XS) % R : rot;
            SK_T(5)   // upsampled MFMA loop
            const bool stay = MIX8 && !f8;   // mix8: the chunk's fp8 phase reads the planes that are staged: nothing to hand over
            if (!stay) __syncthreads();
            SK_T(6)   // barrier
            if (have_next && !stay) {
                if (!last) {
                    if (v_dma(cu + 1)) issue_low(step, cu + 1, false, rot);   // (mix8: cu + 1 is the next chunk's fp16 phase; both halves)
                    prefetch_up(cu + 1);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                } else {
                    issue_fine(step + 1, 0, ring, rot_n);
                    prefetch_skip(0);
                }
            }
            SK_T(7)   // LDS-DMA issue + weight prefetch
            if (last) {
                // ---------------- epilogue (overlaps the DMA): raw fp16 store + GroupNorm partials ------
                char* outw = outb + (long long)x0 * out_plane;
                // the sixteen store offsets of a step are functions of the lane's store voxel alone; hoisted out of the step loop they
                // are held -- in the mix8 form spilled and reloaded -- across every phase (46 registers, +1.5 GB written per 32-tile
                // launch in the PMC pass): formed here, per step
                int ovox_s = ovox;
                asm volatile("" : "+v"(ovox_s));
                const __amdgpu_buffer_rsrc_t rout = sk::make_rsrc(outw, (unsigned)(XS * out_plane));
    #pragma unroll
                for (int o = 0; o < XS; ++o) {
                    const int x = x0 + o;
    #pragma unroll
                    for (int part = 0; part < (SPLIT ? 2 : 1); ++part) {   // SPLIT: the hi halves, then the lo halves
    #pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        unsigned d[2][2];
    #pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const f32x4 r = acc[o][i][j];
                            half4 hv = {(t16)r[0], (t16)r[1], (t16)r[2], (t16)r[3]};
                            if (part == 1)   // lo = fp16(v - hi): exact difference, rounded once
                                hv = half4{(t16)(r[0] - (float)hv[0]), (t16)(r[1] - (float)hv[1]),
                                           (t16)(r[2] - (float)hv[2]), (t16)(r[3] - (float)hv[3])};
                            const uint2 u = __builtin_bit_cast(uint2, hv);
                            d[j][0] = u.x;
                            d[j][1] = u.y;
                            const bool in = vvalid(j) && x < xb;
                            if (SPLIT) {
                                if (part == 0 && in) {   // split: statistics of the fp32 accumulators
                                    gsum[i] += (r[0] + r[1]) + (r[2] + r[3]);
                                    gsq[i] += (r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3]);
                                }
                            } else {
                                const t16x2 z2 = {(t16)0.0f, (t16)0.0f}, one2 = {(t16)1.0f, (t16)1.0f};
                                const t16x2 lo2 = in ? t16x2{hv[0], hv[1]} : z2, hi2 = in ? t16x2{hv[2], hv[3]} : z2;
                                gsum[i] = SK_DOT2_T16(lo2, one2, gsum[i]);
                                gsum[i] = SK_DOT2_T16(hi2, one2, gsum[i]);
                                gsq[i] = SK_DOT2_T16(lo2, lo2, gsq[i]);
                                gsq[i] = SK_DOT2_T16(hi2, hi2, gsq[i]);
                            }
                        }
                        const auto s0 = __builtin_amdgcn_permlane16_swap(d[0][0], d[1][0], false, false);
                        const auto s1 = __builtin_amdgcn_permlane16_swap(d[0][1], d[1][1], false, false);
                        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                        const u32x4 lv = {s0[0], s1[0], s0[1], s1[1]};
                        const bool sok = x < xb && ovox_s >= 0;
                        // split: the voxel line is [hi (cout) | lo (cout)]: out_vs = 4 cout bytes, the lo halves cout * 2 bytes on
                        const unsigned off = (unsigned)(o * (int)out_plane + ovox_s * a.out_vs + part * (a.out_vs / 2) + a.cout_off * 2 +
                                                        32 * i + 16 * (g >> 1));
                        // always issued (the counted wait below relies on it); a masked lane's offset is out of range: dropped
                        __builtin_amdgcn_raw_buffer_store_b128(lv, rout, sok ? off : sk::kOob, 0, 0);
                    }
                    }
                }
                SK_T(8)   // epilogue
                if (have_next) {
                    // vmcnt retires in order: everything older than the epilogue's XS * 2 stores -- the LDS-DMA and the
                    // weight fragments -- has landed (conv3_m16_kernel)
                    constexpr int kStores = XS * 2 * (SPLIT ? 2 : 1);
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kStores) : "memory");
                }
            }
            SK_T(9)   // deferred landing wait
            if (have_next && !stay) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            SK_T(10)  // closing barrier
            rot = rot_n;
        }
    }

    SK_T_DUMP_ROW(a, blockIdx.x < sk::kTimingBlocks, blockIdx.x, w, lane)
    // ---- block-level reduction of the GroupNorm partials ------------------------------------
    if (a.partial) {
        float* red = reinterpret_cast<float*>(lds);
        gn_wave_sum16(red, gsum, gsq, w, c16, g);
        gn_block_sum<1>(red, a.partial, b, nblk, block_in_batch, a.pstride, a.poff, tid);
    }
}

