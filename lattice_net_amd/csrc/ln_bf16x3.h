// The "bf16x3" arithmetic of the large-lattice convolutions (ln_conv.hip, lattices of >= LN_CONV_B3_MIN_ROWS vertices), defined once: the
// exact three-way split of an fp32 operand, the packing of two parts per dword, and the six cross products in their pinned order on
// the bf16 matrix cores.  Device code only.
// fp32-input MFMA runs at the fp32 VECTOR rate on gfx950 (32 cycles per 16x16x4): at ScanNet / SemanticKITTI shapes the fp32 kernel
// sits at 50-80 % of that peak.  Here a = a1 + a2 + a3 EXACTLY, each part the top 16 bits of what is left (bf16 has fp32's
// exponent range, so no scaling; 3 x 8 significant bits = fp32's 24), the same for the filter, and a*b is accumulated in fp32 as
// the six products of total order <= 4: a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1 (what is dropped is < 2^-23 |ab|).  One
// v_mfma_f32_16x16x32_bf16 contracts 32 channels in ~17 cycles, so a slot costs 6 V/32 NT of those instead of V/4 NT of 32
// cycles: 2.5x less matrix time, for ~8 bit operations per gathered value.  The filter bank is split once per call
// (k_conv_split_bank) into fragment order, so staging a slot is a straight 16-byte copy.
// Lane (i, q) holds its quarter of the gathered row, V/4 contiguous channels: MFMA step s takes channels [8s, 8s + 8) of the
// quarter as the A fragment of k-group q, i.e. the contraction order inside a slot is permuted; the bank uses the same order.
#pragma once

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // a matrix-core fragment as it travels: 8 bf16, two per dword

// x = hi + mid + lo exactly, each the top 16 bits of the remainder; returned as raw bf16 bit patterns in the HIGH half-words
// (`lo` comes back UNMASKED — its low half-word is whatever is left below the third part: every user takes the high half-word only, by a
// 16-bit shift or through ln_pack_hi)
__device__ __forceinline__ void ln_split3_bits(float x, unsigned int& hi, unsigned int& mid, unsigned int& lo) {
    hi = __float_as_uint(x) & 0xFFFF0000u;
    const float r1 = x - __uint_as_float(hi);
    mid = __float_as_uint(r1) & 0xFFFF0000u;
    const float r2 = r1 - __uint_as_float(mid);
    lo = __float_as_uint(r2);
}
// two bf16 per dword: the HIGH half-word of `a` in the low half, the high half-word of `b` in the high half — one v_perm_b32 (round 6;
// before: shift + or on masked words, 3 more vector-ALU instructions per pair of split values)
__device__ __forceinline__ unsigned int ln_pack_hi(unsigned int a, unsigned int b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }

// x[at .. at + 8) -> the three fragments p[0] (hi), p[1] (mid), p[2] (lo): two bf16 per dword, the LOWER channel in the low half-word
template <int N>
__device__ __forceinline__ void ln_split3_pack8(const float (&x)[N], int at, u32x4 (&p)[3]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned int h0, m0, l0, h1, m1, l1;
        ln_split3_bits(x[at + 2 * j], h0, m0, l0);
        ln_split3_bits(x[at + 2 * j + 1], h1, m1, l1);
        p[0][j] = ln_pack_hi(h0, h1);
        p[1][j] = ln_pack_hi(m0, m1);
        p[2][j] = ln_pack_hi(l0, l1);
    }
}
// The same split of the 8 floats that arrive as two raw 16-byte LDS reads (the wide forms), written out so that the byte permutes take
// the top half-words of x, r1 and r2 directly: only the two masks the subtractions need are computed.
__device__ __forceinline__ void ln_split3_pack8_raw(const u32x4 (&raw)[2], bf16x8 (&dst)[3]) {
    u32x4 p[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x0 = __uint_as_float(raw[j >> 1][(2 * j) & 3]), x1 = __uint_as_float(raw[j >> 1][(2 * j + 1) & 3]);
        const float r10 = x0 - __uint_as_float(__float_as_uint(x0) & 0xFFFF0000u), r11 = x1 - __uint_as_float(__float_as_uint(x1) & 0xFFFF0000u);
        const float r20 = r10 - __uint_as_float(__float_as_uint(r10) & 0xFFFF0000u), r21 = r11 - __uint_as_float(__float_as_uint(r11) & 0xFFFF0000u);
        p[0][j] = ln_pack_hi(__float_as_uint(x0), __float_as_uint(x1));
        p[1][j] = ln_pack_hi(__float_as_uint(r10), __float_as_uint(r11));
        p[2][j] = ln_pack_hi(__float_as_uint(r20), __float_as_uint(r21));
    }
    dst[0] = __builtin_bit_cast(bf16x8, p[0]), dst[1] = __builtin_bit_cast(bf16x8, p[1]), dst[2] = __builtin_bit_cast(bf16x8, p[2]);
}

// The six products, small terms first, the dominant product last: a3b1, a1b3, a2b2, a2b1, a1b2, a1b1.  The order is part of the
// contract (the 1e-5-against-fp64 bars of the GPU tests are measured with it), and the six issue back to back: an instruction between
// two products on one accumulator costs ~43 cycles (MI355X_MICROARCH.md), so whatever else a kernel has to do goes between chains —
// pinned with scheduling directives at the call site, not here.

// v_mfma_f32_16x16x32_bf16, one accumulation chain
__device__ __forceinline__ void ln_b3_mfma16(const bf16x8 (&a)[3], const bf16x8 (&b)[3], floatx4& acc) {
    const bf16x8 a1 = a[0], a2 = a[1], a3 = a[2], b1 = b[0], b2 = b[1], b3 = b[2];
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b3, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc, 0, 0, 0);
}
// v_mfma_f32_32x32x16_bf16, N chains that share A and advance together (product p of every column tile, then product p + 1)
template <int N>
__device__ __forceinline__ void ln_b3_mfma32(const bf16x8 (&a)[3], const u32x4 (&b)[N][3], floatx16 (&acc)[N]) {
#define LN_B3_P32(PA, PB)                                                                                                                     \
    _Pragma("unroll") for (int nt = 0; nt < N; ++nt)                                                                                          \
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA], __builtin_bit_cast(bf16x8, b[nt][PB]), acc[nt], 0, 0, 0);
    LN_B3_P32(2, 0) LN_B3_P32(0, 2) LN_B3_P32(1, 1) LN_B3_P32(1, 0) LN_B3_P32(0, 1) LN_B3_P32(0, 0)
#undef LN_B3_P32
}
