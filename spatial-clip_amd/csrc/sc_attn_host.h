// Host side of the attention layer: what a call is (shape + operands), what every kernel file exports (an acceptance
// predicate and a launch function) and the launch helpers they share.  The table that orders the paths, the planner that
// walks it and sc_attn_fwd / sc_attn_bwd are in sc_attention.hip.
#pragma once
#include "sc_common.h"
#include "sc_kernels.h"
#include <type_traits>
#include <utility>

// One validated call: B, H, L > 0, 1 <= Lq <= L (the query rows that are computed), dh in {32, 64, 80}.
struct AttnShape {
    int B, L, Lq, H, dh, causal;
    int nheads() const { return B * H; }
    float scale() const { return 1.0f / sqrtf((float)dh); }
    long long out_bytes() const { return (long long)B * L * H * dh * 2; }    // out  [B*L, H*dh] bf16
    long long lse_bytes() const { return (long long)B * H * L * 4; }         // lse  [B, H, L] fp32
    long long dqkv_bytes() const { return 3 * out_bytes(); }                 // dqkv [B*L, 3*H*dh] bf16
};
struct AttnFwdOps {
    const bf16* qkv;
    bf16* out;
    float* lse;
};
struct AttnBwdOps {
    const bf16 *qkv, *out, *dout;
    const float* lse;
    float* delta;
    bf16* dqkv;
};

// Every path: `accepts` is a pure function of the shape (no HIP call, no environment) that includes the kernel's LDS,
// wave-count and byte-size limits; `launch` assumes acceptance and returns 0, or < 0 with sc_last_error set.
#define SC_ATTN_PATH(NAME, OPS)                 \
    bool sc_attn_##NAME##_accepts(const AttnShape& s); \
    int sc_attn_##NAME##_launch(const AttnShape& s, const OPS& o, hipStream_t st);
SC_ATTN_PATH(fwd_stream, AttnFwdOps)        // sc_attention_stream.hip: K / V streamed through LDS in 64-row tiles
SC_ATTN_PATH(fwd_persistent, AttnFwdOps)    // sc_attention_p.hip: persistent workgroups, LDS-DMA double buffering, L <= 224
SC_ATTN_PATH(fwd_persistent2, AttnFwdOps)   // sc_attention_p2.hip: the same for 224 < L <= 288, two query tiles per wave
SC_ATTN_PATH(bwd_cls, AttnBwdOps)           // sc_attention_cls.hip: q_rows == 1 (class-token-only last block), any L
SC_ATTN_PATH(bwd_stream, AttnBwdOps)        // sc_attention_stream.hip: dq + dkv, Q / dO (K / V) streamed
SC_ATTN_PATH(bwd_ring, AttnBwdOps)          // sc_attention_bwd3.hip: single pass, dQ by MFMA chains over a ring of dS tiles
SC_ATTN_PATH(bwd_ring8, AttnBwdOps)         // sc_attention_bwd4.hip: the ring design for 224 < L <= 257, eight key waves
SC_ATTN_PATH(bwd_single_pass, AttnBwdOps)   // sc_attention_bwd1.hip: single pass, dQ accumulated in LDS
SC_ATTN_PATH(bwd_persistent, AttnBwdOps)    // sc_attention_bwd2.hip: persistent two-pass with loader waves (also causal)
#undef SC_ATTN_PATH

constexpr size_t ATTN_LDS_MAX = 160 * 1024;      // LDS of a CU: a workgroup's dynamic allocation stops here

// The persistent kernels address out / lse / dqkv through a buffer resource: 32-bit byte offsets, and 0xFFFFFFF0 is the
// offset they give a masked lane, so the tensor has to end below it.
inline bool attn_fits_buffer(long long bytes) { return bytes < 0xFFFFFFF0ll; }

// min(nheads, CUs): one workgroup per CU walks a list of heads.  0 with sc_last_error set when the device cannot be
// queried (sc_attention.hip; the CU count is read once).
int attn_persistent_grid(int nheads);
// measurement switch of the two ring kernels: SC_ATTN_GRID=<n> caps the number of workgroups
int attn_grid_cap(int grid);

// raises the kernel's dynamic-LDS limit to `lds` bytes (kernels with static LDS pass 0) and launches it
template <class... P, class... A>
void attn_launch(void (*kernel)(P...), unsigned grid, int threads, size_t lds, hipStream_t st, A... args) {
    if (lds)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    kernel<<<grid, threads, lds, st>>>(args...);
}

// Run-time value -> template argument: calls f(std::integral_constant<int, V>{}) for the V of the list that equals v
// (false when none does); with two lists, f(A, B).  A generic lambda names the kernel: attn_kernel<A.value, B.value>.
template <int... Vs>
using attn_vals = std::integer_sequence<int, Vs...>;
template <int... Vs, class F>
bool attn_dispatch(attn_vals<Vs...>, int v, F&& f) {
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}
template <int... As, int... Bs, class F>
bool attn_dispatch(attn_vals<As...> as, int a, attn_vals<Bs...> bs, int b, F&& f) {
    return attn_dispatch(as, a, [&](auto A) { attn_dispatch(bs, b, [&](auto B) { f(A, B); }); });
}
// The lists are written last value first: the compiler emits the kernels a lambda names in the reverse of the list, and a
// change of the host code is checked by comparing the disassembly of the code object, kernel order included.
using attn_blocks7 = attn_vals<7, 6, 5, 4, 3, 2, 1>;     // 32-key blocks of the kernels that stop at 224 tokens
using attn_causal = attn_vals<0, 1>;
