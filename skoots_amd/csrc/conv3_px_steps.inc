// The step machinery that conv3_px_kernel and conv3_pxm_kernel share, included inside both kernel bodies: the bias reset, the
// tap addresses, the weight fragments and the pair step over two input planes.  Text inclusion, not functions: as
// force-inlined free functions the same code changed the register allocation of both kernels and left conv3_px_kernel
// with a 16-byte spill (tools/kernel_isa_diff.py); included, it compiles to the instructions each kernel had with its own
// copy.  Takes lds, plane_bytes, zero_addr, needed, lane, g, q_row, pitch, zlo, zhi, wres, wlds, RESH from the including kernel.
// the bias (the accumulators' initial value) is re-read from its copy in LDS -- padding positions of slot 1 -- at every
// reset: eight registers less in the loop
const float* lbias = reinterpret_cast<const float*>(lds + plane_bytes + needed * kPosBytes) + 4 * g;
auto reset = [&](f32x4 (&o)[2][2]) {
    o[0][0] = o[0][1] = *reinterpret_cast<const f32x4*>(lbias);
    o[1][0] = o[1][1] = *reinterpret_cast<const f32x4*>(lbias + 16);
};
auto baddr = [&](int dydz, int j) -> int {
    const int dz = dydz % 3 - 1;
    const int q = q_row + (dydz / 3 - 1) * pitch + dz;
    int addr = (q * 4 + (g ^ (((q >> 2) & 1) << 1))) * 16 + 1024 * j;
    if (dz < 0) addr = zlo(j) ? zero_addr + (addr & 255) : addr;
    if (dz > 0) addr = zhi(j) ? zero_addr + (addr & 255) : addr;
    return addr;
};
auto wfrag = [&](int dydz, int i, half8 (&dst)[3]) {
    if (2 * dydz + i < RESH) {
#pragma unroll
        for (int d = 0; d < 3; ++d) dst[d] = wres[2 * dydz + i][d];
    } else {
        const char* p = wlds + (2 * dydz + i - RESH) * 3 * 1024 + lane * 16;
#pragma unroll
        for (int d = 0; d < 3; ++d) dst[d] = *reinterpret_cast<const half8*>(p + d * 1024);
    }
};

// A step over the input planes A (slot sA) and B = A + 1 (slot sB).  oA1 / oA / oB / oB1: the accumulators of the
// output planes A-1, A, B, B+1.  Tap d of a weight row multiplies x_in = x_out + d - 1.
auto pair_step = [&](auto SA, auto SB, f32x4 (&oA1)[2][2], f32x4 (&oA)[2][2], f32x4 (&oB)[2][2], f32x4 (&oB1)[2][2]) {
    // compile-time slots: the 18 tap addresses of the patch (plane-relative, loop-invariant) serve both planes of
    // every step through the immediate offset of ds_read_b128
    const char* pa = lds + decltype(SA)::value * plane_bytes;
    const char* pb = lds + decltype(SB)::value * plane_bytes;
    half8 bq[2][2][2];   // [buffer][plane][j]: the B fragments of a tap row, one row ahead
    half8 wq[2][3];      // [buffer][d]: the weight fragments of a half row (cout half i of a tap row), one half row ahead
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ad = baddr(0, j);
        bq[0][0][j] = *reinterpret_cast<const half8*>(pa + ad);
        bq[0][1][j] = *reinterpret_cast<const half8*>(pb + ad);
    }
    wfrag(0, 0, wq[0]);
    // The 18 half rows of a step, 12 MFMAs each (192 cycles of the matrix pipe).  The LDS reads of half row h + 1 -- its
    // three weight fragments when its tap row lives in LDS, and the four B fragments of the next tap row -- are issued
    // in the FIRST MFMA gaps of half row h, in the order half row h + 1 consumes them, so the youngest read is 80+
    // cycles old (and not needed before the seventh MFMA) when half row h + 1 starts.  The order is pinned: left to
    // itself the scheduler spread the reads to the END of the half row and every half row began with an
    // `s_waitcnt lgkmcnt(0)` on a read issued one MFMA earlier (SQ_WAIT_ANY 38 % of the wave-cycles).
#pragma unroll
    for (int dydz = 0; dydz < 9; ++dydz) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int h = dydz * 2 + i;   // its weights sit in wq[h & 1], its B fragments in bq[dydz & 1]
            const half8(&W)[3] = wq[h & 1];
            const int ndy = i == 0 ? dydz : dydz + 1, ni = i ^ 1;         // the next half row
            bool wread = ndy < 9 && 2 * ndy + ni >= RESH;                  // ... reads its weights from LDS
            bool bread = i == 1 && dydz < 8;                               // ... starts a new tap row: B fragments
            if (SK_PX_ABL(16) && wread) {   // timing experiment: no LDS weight reads (a resident half row instead)
                wread = false;
                wfrag((2 * ndy + ni) % RESH / 2, (2 * ndy + ni) % RESH % 2, wq[(h + 1) & 1]);
            } else if (ndy < 9 && !wread) {
                wfrag(ndy, ni, wq[(h + 1) & 1]);                           // resident row: register names only
            }
            if (SK_PX_ABL(32) && bread) {   // timing experiment: no B fragment reads after the first tap row
                bread = false;
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) bq[(dydz + 1) & 1][pl][jj] = bq[dydz & 1][pl][jj];
            }
            // read k of the next half row, in consumption order: W0, A0, B0, W1, W2, A1, B1
            auto next_read = [&](int k) {
                const char* wp = wlds + (2 * ndy + ni - RESH) * 3 * 1024 + lane * 16;
                int kk = k;
                if (!wread) kk = (k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 5 : 6);   // B fragments only: A0, B0, A1, B1
                if (!bread && kk > 0) kk = (kk == 1 ? 3 : 4);                  // weights only: W0, W1, W2
                switch (kk) {
                    case 0: wq[(h + 1) & 1][0] = *reinterpret_cast<const half8*>(wp); break;
                    case 1: bq[(dydz + 1) & 1][0][0] = *reinterpret_cast<const half8*>(pa + baddr(dydz + 1, 0)); break;
                    case 2: bq[(dydz + 1) & 1][1][0] = *reinterpret_cast<const half8*>(pb + baddr(dydz + 1, 0)); break;
                    case 3: wq[(h + 1) & 1][1] = *reinterpret_cast<const half8*>(wp + 1024); break;
                    case 4: wq[(h + 1) & 1][2] = *reinterpret_cast<const half8*>(wp + 2048); break;
                    case 5: bq[(dydz + 1) & 1][0][1] = *reinterpret_cast<const half8*>(pa + baddr(dydz + 1, 1)); break;
                    default: bq[(dydz + 1) & 1][1][1] = *reinterpret_cast<const half8*>(pb + baddr(dydz + 1, 1)); break;
                }
            };
            const int nreads = (wread ? 3 : 0) + (bread ? 4 : 0);
#pragma unroll
            for (int m = 0; m < 12; ++m) {
                const int j = m / 6;
                const half8 fa = bq[dydz & 1][0][j], fb = bq[dydz & 1][1][j];
                switch (m % 6) {   // tap d of a weight row multiplies x_in = x_out + d - 1
                    case 0: oB[i][j] = SK_MFMA_16x16x32_T16(W[0], fa, oB[i][j], 0, 0, 0); break;
                    case 1: oB1[i][j] = SK_MFMA_16x16x32_T16(W[0], fb, oB1[i][j], 0, 0, 0); break;
                    case 2: oA[i][j] = SK_MFMA_16x16x32_T16(W[1], fa, oA[i][j], 0, 0, 0); break;
                    case 3: oA1[i][j] = SK_MFMA_16x16x32_T16(W[2], fa, oA1[i][j], 0, 0, 0); break;
                    case 4: oB[i][j] = SK_MFMA_16x16x32_T16(W[1], fb, oB[i][j], 0, 0, 0); break;
                    default: oA[i][j] = SK_MFMA_16x16x32_T16(W[2], fb, oA[i][j], 0, 0, 0); break;
                }
                if (m < nreads) next_read(m);
                if (m <= nreads) __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};
