// Weight staging of conv3_px_kernel and conv3_pxm_kernel (+ the zero windows and the bias), included inside both kernel
// bodies (text inclusion, not a function: see conv3_px_steps.inc).  Takes a, lds, tid, lane, needed, plane_bytes, zero_addr,
// NSLOT, RESH and the weights' buffer resource wrsrc from the including kernel.
// ---- weights: half rows (tap row dydz, cout half i) 0 .. RESH-1 in registers, RESH .. 17 in LDS behind the ring ----
// fragment of (row dydz, cout half i, x tap d): ((dydz * 2 + i) * 3 + d) KiB into the packed weight
half8 wres[RESH][3];
#pragma unroll
for (int r = 0; r < RESH; ++r)
#pragma unroll
    for (int d = 0; d < 3; ++d)
        wres[r][d] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, lane * 16, (r * 3 + d) * 1024, 0));
char* wlds = lds + NSLOT * plane_bytes;
for (int i = tid; i < (18 - RESH) * 3 * 64; i += 256)
    *reinterpret_cast<uint4*>(wlds + i * 16) = *reinterpret_cast<const uint4*>(a.wpk + RESH * 3 * 1024 + i * 16);
// padding positions of a slot: needed, needed + 1 (128 bytes: slot 0 the GroupNorm scales of a raw source, slot 1 the
// bias, slot 2 the GroupNorm shifts) | the zero window NPOSP - 4 .. NPOSP - 1
if (tid < NSLOT * 16)
    *reinterpret_cast<uint4*>(lds + (tid >> 4) * plane_bytes + zero_addr + (tid & 15) * 16) = make_uint4(0, 0, 0, 0);
if (tid >= 128 && tid < 160) reinterpret_cast<float*>(lds + plane_bytes + needed * kPosBytes)[tid - 128] = a.bias[tid - 128];
