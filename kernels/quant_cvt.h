// Exact int8 / int4-g128 -> bf16 weight conversion shared by the kernels that
// dequantise on the fly (gemm_tile_q.hip, moe_gemm_q.hip).
//
// A weight byte b in offset-binary (int4 nibble: q+8; int8: q+128 after
// flipping the sign bit) is converted with v_cvt_f32_ubyte and one
// fma(b, s, -off*s).  off*s is exact (power-of-two multiple) and the fma
// rounds the exact product q*s once, so the f32 equals torch's q.float()*s;
// v_cvt_pk_bf16_f32 then rounds to nearest even as torch's .to(bf16) does.
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;

#define TQ_BN 128
#define TQ_BK 64
#define TQ_GROUP 128  // int4 scale group along K

// skewed byte offset of (row, k8 slot) in a [rows][64] bf16 image
DEVINLINE int tq_swz(int row, int k8) {
  return row * (TQ_BK * 2) + (((k8 + (row >> 1)) & 7) << 4);
}

DEVINLINE unsigned tq_pk_bf16(float a, float b) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// byte i of u -> (byte - off) * s with c = -off * s, exact (see header)
template <int I>
DEVINLINE float tq_byte(unsigned u, float s, float c) {
  return __builtin_fmaf((float)((u >> (8 * I)) & 0xFFu), s, c);
}

// one dword of int4 storage (8 weights) -> 8 bf16
DEVINLINE u32x4_t tq_dq4(unsigned u, float s, float c) {
  const unsigned lo = u & 0x0F0F0F0Fu;         // weights 0,2,4,6
  const unsigned hi = (u >> 4) & 0x0F0F0F0Fu;  // weights 1,3,5,7
  u32x4_t o;
  o[0] = tq_pk_bf16(tq_byte<0>(lo, s, c), tq_byte<0>(hi, s, c));
  o[1] = tq_pk_bf16(tq_byte<1>(lo, s, c), tq_byte<1>(hi, s, c));
  o[2] = tq_pk_bf16(tq_byte<2>(lo, s, c), tq_byte<2>(hi, s, c));
  o[3] = tq_pk_bf16(tq_byte<3>(lo, s, c), tq_byte<3>(hi, s, c));
  return o;
}

// two dwords of int8 storage (8 weights) -> 8 bf16
DEVINLINE u32x4_t tq_dq8(unsigned u0, unsigned u1, float s, float c) {
  u0 ^= 0x80808080u;  // two's complement -> offset-binary (q + 128)
  u1 ^= 0x80808080u;
  u32x4_t o;
  o[0] = tq_pk_bf16(tq_byte<0>(u0, s, c), tq_byte<1>(u0, s, c));
  o[1] = tq_pk_bf16(tq_byte<2>(u0, s, c), tq_byte<3>(u0, s, c));
  o[2] = tq_pk_bf16(tq_byte<0>(u1, s, c), tq_byte<1>(u1, s, c));
  o[3] = tq_pk_bf16(tq_byte<2>(u1, s, c), tq_byte<3>(u1, s, c));
  return o;
}
