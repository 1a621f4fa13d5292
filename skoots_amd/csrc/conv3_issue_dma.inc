// issue_dma of conv3_kernel and conv3_m16_kernel, included inside both kernel bodies: the LDS-DMA of the planes x0 - 1 ..
// x0 + XS of phase chunk `ch` of the step at x0 = xa + step * XS into the ring slots (rot_n + i) % R.  Text inclusion, not a
// function: as a force-inlined free function the same code changed the register allocation of every variant of both
// kernels (tools/kernel_isa_diff.py).  Takes a, lds, plane_bytes, xa, b, w, ndma, d_cs, d_vox, d_up, XS, R from the kernel.
// buffer-resource LDS-DMA and stores: 32-bit offsets into this batch item's tensors (one address VGPR instead of
// two, 32-bit address arithmetic: -2 % time); an out-of-range offset reads zeros -- what the halo / padding lanes
// want -- and drops a masked store
// A descriptor covers only the x-planes of ONE step (built per phase from wave-uniform values: a few scalar
// instructions): a tensor of one batch item may exceed the 4 GiB a descriptor / a 32-bit offset can span
// (the split mode's 512x512x128 tile: 4.3 GB per 32-channel tensor).
auto issue_dma = [&](int step, int ch, bool reuse, int rot_n) {
    const int x0 = xa + step * XS;
    const unsigned ci = a.chinfo[ch];
    const int si = ci & 1;
    const SrcDev s = a.src[si];
    const int choff = ci >> 8;  // byte offset of the chunk in the voxel line
    const int first_new = reuse ? 2 : 0;  // planes 0,1 are the previous phase's planes XS, XS + 1
    const int xlo = s.up ? (max(x0 - 1, 0) >> 1) : max(x0 - 1, 0);   // first source plane of the step
    const long long wbytes = min((long long)(R + 1) * s.plane, s.batch - (long long)xlo * s.plane);
    const __amdgpu_buffer_rsrc_t rsrc = sk::make_rsrc(s.data + (long long)b * s.batch + (long long)xlo * s.plane, (unsigned)wbytes);
    for (int i = SK_ABL(a, 1) ? R : first_new; i < R; ++i) {
        const int x = x0 - 1 + i;
        const int slotp = (rot_n + i) % R;
        const bool xok = x >= 0 && x < a.Xt;
        char* lbase = lds + slotp * plane_bytes;
        const unsigned xoff = (unsigned)(((s.up ? (x >> 1) : x) - xlo) * (int)s.plane + choff + d_cs);
        const unsigned vstride = (unsigned)(s.C * 2);
#pragma unroll
        for (int k = 0; k < kMaxDma; ++k) {
            const int t = w + 4 * k;
            if (t < ndma) {
                const int vox = s.up ? d_up[k] : d_vox[k];
                const unsigned voff = (xok && vox >= 0) ? xoff + (unsigned)vox * vstride : sk::kOob;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lbase + t * 1024), 16, voff, 0, 0, 0);
            }
        }
    }
};
