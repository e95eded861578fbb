// The device primitives every f16x3 kernel shares: the vector types, the fp32 -> (hi, lo) operand split, the three-pass MFMA product
// and the raw-buffer resource.  This is the arithmetic the 1e-3 contract rests on: x = hi + lo with hi = fp16(x),
// lo = fp16(x - hi) (22 significant bits), products accumulated as lo*hi + hi*lo + hi*hi in the fp32 MFMA accumulator.
// Not here on purpose: the single-pass ("f16", NPASS == 1) paths round to nearest and have no lo half, and the 16x16x32 forms issue
// their passes per 16x16 sub-tile -- both stay with the kernels that own them.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ void otvm_split4(const f32x4 v, f16x4& hi, f16x4& lo) {
    // hi: round-toward-zero pack (any rounding works, lo is computed exactly against it)
    typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));
    const fp16x2 p01 = __builtin_amdgcn_cvt_pkrtz(v.x, v.y);
    const fp16x2 p23 = __builtin_amdgcn_cvt_pkrtz(v.z, v.w);
    const f16x2 h01 = __builtin_bit_cast(f16x2, p01);
    const f16x2 h23 = __builtin_bit_cast(f16x2, p23);
    hi = f16x4{h01.x, h01.y, h23.x, h23.y};
    lo = f16x4{(_Float16)(v.x - (float)h01.x), (_Float16)(v.y - (float)h01.y), (_Float16)(v.z - (float)h23.x),
               (_Float16)(v.w - (float)h23.y)};
}

// (the scalar form rounds hi to nearest: one conversion instead of a pack; lo is exact against it all the same)
static __device__ __forceinline__ void otvm_split1(float v, _Float16& hi, _Float16& lo) {
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}

// ACC += A * B on v_mfma_f32_32x32x16_f16 in three passes, the small terms first: lo*hi, hi*lo, hi*hi (lo*lo, 2^-22 relative, is dropped)
#define OTVM_MFMA3(ACC, AH, AL, BH, BL)                                         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(AL, BH, ACC, 0, 0, 0);         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(AH, BL, ACC, 0, 0, 0);         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(AH, BH, ACC, 0, 0, 0)

// Raw buffer resource over [p, p + bytes): an access at an offset >= bytes reads zeros and moves no data, which is how the kernels
// load padding without a branch.  Flags word (dword 3 of the descriptor): DATA_FORMAT = 32-bit (bits 15-18 = 4), stride 0, nothing else set.
constexpr int OTVM_BUFFER_RSRC_FLAGS = 0x00020000;
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t otvm_buffer_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, OTVM_BUFFER_RSRC_FLAGS);
}
