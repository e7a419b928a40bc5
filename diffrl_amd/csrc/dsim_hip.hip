// dsim_hip.hip -- gfx950 kernels + the C ABI of include/dsim.h.
//
// Mapping: ONE environment per workgroup.  The phase code of an environment runs on ONE wavefront (64 lanes) -- plus, while
// all environments of a launch are resident at once, a HELPER wavefront that executes only the side blocks of split phases
// (DevExec<..., HELPER>) -- or on four wavefronts for models whose item lists are several wavefronts long (muscles).  The
// articulation template (a few KB) is copied from global memory into LDS once per launch, the environment's state row is
// loaded with one coalesced read per tensor, all `substeps` substeps run out of LDS, and only (q, qd) [+ the per-substep
// checkpoint when gradients are wanted] go back to HBM.  N=1024 environments put one main wave on each of the 1024 SIMDs
// of an MI355X; larger N stacks waves per SIMD and hides LDS/VALU latency.
//
// Every kernel exists in a GENERIC form (LDS offsets and model sizes are runtime values in SGPRs) and in
// per-model SPECIALISED forms (dsim_static_layouts.hpp: offsets are instruction immediates, sizes are
// compile-time loop bounds).  dsim_model_create picks a specialised form only if the layout it builds at
// run time is bit-identical to the generated table; the first profile of the generic kernels showed that
// >60 % of their instruction stream was SGPR spilling (v_readlane/v_writelane), address arithmetic and
// moves caused by ~100 runtime offsets (profiles/r01_*), which is what the specialisation removes.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC dsim_hip.hip -o libdsim_hip.so
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <new>
#include <string>
#include <tuple>

#define DSIM_FN __device__ __forceinline__
#ifndef DSIM_OPAQUE
#define DSIM_OPAQUE(x) asm volatile("" : "+v"(x))
#endif
#include "dsim_core.hpp"
#include "dsim_abi.hpp"
#define DSIM_LIT_FN __device__ inline
#include "dsim_literal.hpp"
#ifdef DSIM_STATIC_LAYOUTS_FILE   // (python -m diffrl_amd.specialise --header-out: a generated header outside the tree)
#include DSIM_STATIC_LAYOUTS_FILE
#else
#include "dsim_static_layouts.hpp"
#endif

namespace {

// The workgroup IS one wavefront (64 threads, enforced at launch): a phase boundary needs no s_barrier and no wait at all.
// The DS instructions of one wave are executed by the LDS in issue order, so a load issued after a store observes it
// whichever lanes are involved; the only requirement is that the COMPILER does not move or cache LDS accesses across the
// boundary -- an empty asm with a memory clobber.  (Round 1 / early round 2 drained the queue with `s_waitcnt lgkmcnt(0)`
// here: every phase then paid the latency of its last store before the next phase's loads could even be issued; without
// it the results are bit-identical and Ant 1024 runs 1.7 % faster.  -DDSIM_WAVE_SYNC_ASM='"s_waitcnt lgkmcnt(0)"' builds
// the draining variant for A/B runs.)  Global loads / stores (vmcnt) are never waited for here either, which is what
// lets checkpoint traffic overlap with compute.
#ifndef DSIM_WAVE_SYNC_ASM
#define DSIM_WAVE_SYNC_ASM ""
#endif
__device__ __forceinline__ void dsim_wave_sync() { asm volatile(DSIM_WAVE_SYNC_ASM ::: "memory"); }

// reciprocal of a pivot: v_rcp_f32 + one Newton step (< 1 ulp on the pivots of an SPD matrix; ~3 instead of the ~11 instructions
// of the correctly rounded division on the pivot's dependent chain)
__device__ __forceinline__ float dsim_pivot_rcp(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
}
// Gauss-Jordan inverse with lane i holding row i in registers.  Per pivot k the classical in-place update is
//   row k <- p = (row k with column k := 1) / h_kk;  row i <- (row i with column k := 0) - h_ik p        (dsim_core.hpp: dsim_fwd_mass)
// i.e. per column: broadcast h_kj, scale it, multiply-add, select the pivot row: four instructions (round 5 measured the
// deferred form below at -1 % .. -7 % of the forward launch against it, Ant .. SNUHumanoid).  The pivot
// row's scaling commutes with every LATER row operation (they are linear in the row), so lane k keeps its row UNSCALED -- column k
// set to 1 -- remembers 1 / h_kk and scales once at the end; every other row takes f h_kj with f = h_ik / h_kk, lane k with f = 0:
// per column one v_readlane and one multiply-add, no select.  Same elimination, different rounding (f h_kj instead of
// h_ik (h_kj / h_kk)); the generic kernels keep the classical form, the tests hold both to the reference.
template <int N, int NW> __device__ __forceinline__ void dsim_wave_gj(float* H) {
    const int lane = (int)threadIdx.x;
    if (NW > 1 && lane >= DSIM_NL) return;
    const int r = lane < N ? lane : 0;  // idle lanes shadow row 0; they store nothing
    float row[N];
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] = H[r * N + j];
    float scale = 1.0f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float piv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(row[k]), k));
        const float rp = dsim_pivot_rcp(piv);
        const bool own = lane == k;
        const float f = own ? 0.0f : row[k] * rp;
        scale = own ? rp : scale;
        row[k] = own ? 1.0f : 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float hkj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(row[j]), k));
            row[j] = __builtin_fmaf(-f, hkj, row[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] *= scale;
    if (lane < N) {
#pragma unroll
        for (int j = 0; j < N; ++j) H[lane * N + j] = row[j];
    }
}

// The same for a RUN-TIME size n <= NB (generic kernels: no compile-time nd): the matrix is padded with an identity block to
// NB x NB in registers -- lane i < n holds (row i, zeros), lane i >= n the unit row e_i -- so the padded pivots are 1, their
// multipliers 0, and the leading n x n block of the result is H^-1.  NB pivots of NB columns instead of 2 n phases of LDS round
// trips (round 5: the generic Ant forward launch spent 39 k of its 273 k cycles in those phases).
template <int NB, int NW> __device__ __forceinline__ void dsim_wave_gj_pad(float* H, int n) {
    const int lane = (int)threadIdx.x;
    if (NW > 1 && lane >= DSIM_NL) return;
    float row[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) row[j] = (lane < n && j < n) ? H[lane * n + j] : ((j == lane) ? 1.0f : 0.0f);
    float scale = 1.0f;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const float piv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(row[k]), k));
        const float rp = dsim_pivot_rcp(piv);
        const bool own = lane == k;
        const float f = own ? 0.0f : row[k] * rp;
        scale = own ? rp : scale;
        row[k] = own ? 1.0f : 0.0f;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const float hkj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(row[j]), k));
            row[j] = __builtin_fmaf(-f, hkj, row[j]);
        }
    }
    if (lane < n) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if (j < n) H[lane * n + j] = row[j] * scale;
    }
}

// The same for two environments per wavefront (rows of the second one in lanes 32 ..): the pivot row travels through the LDS
// crossbar (ds_bpermute), whose source lane may differ between the halves.
template <int N> __device__ __forceinline__ void dsim_half_gj(float* H, int lane, int half_addr) {
    const int r = lane < N ? lane : 0;
    float row[N];
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] = H[r * N + j];
    float scale = 1.0f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int src = (k << 2) + half_addr;
        const float piv = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(row[k])));
        const float rp = dsim_pivot_rcp(piv);
        const bool own = lane == k;
        const float f = own ? 0.0f : row[k] * rp;
        scale = own ? rp : scale;
        row[k] = own ? 1.0f : 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float hkj = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(row[j])));
            row[j] = __builtin_fmaf(-f, hkj, row[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] *= scale;
    if (lane < N) {
#pragma unroll
        for (int j = 0; j < N; ++j) H[lane * N + j] = row[j];
    }
}

// The LDS image of one environment: [model constants | work arrays].  load(): the constants are copied from global memory
// (16 bytes per lane and load: const_words is a multiple of 4, both sides are 16-byte aligned) and the work area starts
// out as zeros, not as what the previous workgroup on this CU left behind: the weighted range sums (dsim_core.hpp:
// dsim_range_sum_m) multiply entries past the end of a range by 0, which needs them to be finite, and a few spare words
// (the "zero dof" behind atau) are constants 0 that no phase ever writes.
// request() / land(): the copy in two halves, so that the step functions can put their own early loads between them --
// memory returns loads in the order they were issued: constants first (needed first), then the step's inputs.  CW is the
// compile-time const_words of a specialised kernel (the constants wait in CW / 4 / lanes 16-byte registers) or 0 (generic
// kernels: request() does nothing, land() copies).
template <int NW, int CW, int EPW = 1> struct DsimImage {
    typedef float v4f __attribute__((ext_vector_type(4)));
    static constexpr int NLW = DSIM_NL * NW / EPW, REGS = (CW / 4 + NLW - 1) / NLW;
    // lane of this environment (EPW == 2: two environments per wavefront, 32 lanes each; `lds` then differs between the halves)
    static __device__ __forceinline__ int lane_() { return EPW == 1 ? (int)threadIdx.x : (int)(threadIdx.x & (NLW - 1)); }
    float* lds;    // where the constants go
    float* work;   // image base of the work arrays (== lds, except for the second environment of a pair)
    const uint32_t* cblob;
    int const_words, image_words;   // image_words: forward kernels fwd_words, adjoint kernels total_words
    v4f regs[REGS > 0 ? REGS : 1];
    __device__ __forceinline__ void request() {
        if constexpr (CW > 0) {
            const v4f* g = reinterpret_cast<const v4f*>(cblob);
#pragma unroll
            for (int r = 0; r < REGS; ++r) {
                const int i = lane_() + NLW * r;
                if (i < CW / 4) regs[r] = g[i];
            }
        }
    }
    __device__ __forceinline__ void land() {
        v4f* l = reinterpret_cast<v4f*>(lds);
        if constexpr (CW > 0) {
#pragma unroll
            for (int r = 0; r < REGS; ++r) {
                const int i = lane_() + NLW * r;
                if (i < CW / 4) l[i] = regs[r];
            }
        } else {
            const v4f* g = reinterpret_cast<const v4f*>(cblob);
            for (int i = lane_(); i < const_words / 4; i += NLW) l[i] = g[i];
        }
        v4f* w = reinterpret_cast<v4f*>(work);
        for (int i = const_words / 4 + lane_(); i < image_words / 4; i += NLW) w[i] = v4f{0.f, 0.f, 0.f, 0.f};
    }
};

// NW wavefronts per environment (workgroup of 64 * NW lanes).  NW == 1: a phase boundary is the compiler fence above;
// NW > 1: a workgroup barrier (phases whose item count exceeds 64 -- muscles, contacts, matrix entries of the bigger
// models -- are spread over the waves, which sit on different SIMDs of the CU).
// PF: 16-byte prefetch registers per lane for one checkpoint row (specialised kernels: exactly what the model's row needs)
// HELPER: a second wavefront per environment that executes nothing but the side tasks the phase code hands it with
// fork_join (contacts next to links in the kinematics, contacts^T next to the body-level cotangents, ...): those are
// blocks of a phase that run on OTHER LANES WITH DIFFERENT CODE than the phase's main block, which a single wavefront
// can only execute one after the other.  Unlike NW > 1 (every wave runs every phase on its share of the items) the
// helper skips all ordinary phases, so it adds almost nothing to the issue load of the SIMD it shares with another
// environment's main wave; a workgroup barrier of two waves costs ~30 cycles (measured), two per fork_join.
#ifdef DSIM_STAMPS
// developer builds only (tools/stamps.py): cycle stamps of workgroup 0's main wave at every phase boundary of the PRODUCT
// executor (helper wave and all), read back with dsim_debug_stamps.  clock64 is an SMEM read: it drains the wave's LDS queue.
__device__ long long g_dsim_stamps[2 * 16384];
#endif
// EPW == 2: TWO environments per wavefront, 32 lanes each (launches far beyond one wave per SIMD, where the SIMDs are saturated
// and every instruction of a wave whose phases use 9 .. 32 lanes is half wasted).  The phase code is the same: it sees NL = 32
// lanes and an LDS image pointer that differs between the halves; the cross-lane primitives stay inside the half.
template <int NW, int PF = 6, int CW = 0, bool HELPER = false, int EPW = 1> struct DevExec {
    static_assert(EPW == 1 || (EPW == 2 && NW == 1 && !HELPER), "two environments per wavefront: one-wave mapping, no helper");
    static constexpr int ENVS_PER_WAVE = EPW;
#ifdef DSIM_STAMPS
    int stamp_i_ = 0, stamp_tag_ = 0;
    // main wave: entries [0, 8192), helper wave: [8192, 16384) (its tags + 50)
    __device__ __forceinline__ void stamp() {
        // (several wavefronts per environment: the second track is the SECOND wavefront's first lane)
        const bool main_lane = threadIdx.x == 0, help_lane = (HELPER || NW > 1) && threadIdx.x == DSIM_NL;
        if (blockIdx.x == 0 && (main_lane || help_lane) && stamp_i_ < 8192) {
            const int k = stamp_i_ + (help_lane ? 8192 : 0);
            g_dsim_stamps[k] = clock64();
            g_dsim_stamps[16384 + k] = stamp_tag_ + (help_lane ? 50 : 0);
        }
        ++stamp_i_;
        ++stamp_tag_;
    }
    __device__ __forceinline__ void mark(int t) { stamp_tag_ = t * 100; }
#else
    __device__ __forceinline__ void stamp() {}
    __device__ __forceinline__ void mark(int) {}
#endif
    static_assert(!HELPER || NW == 1, "the helper wavefront belongs to the one-wave mapping");
    static constexpr bool HAS_HELPER = HELPER;
    const bool helper_ = HELPER && threadIdx.x >= DSIM_NL;
    __device__ __forceinline__ int lane_() const { return (HELPER || EPW > 1) ? (int)(threadIdx.x & (NL - 1)) : (int)threadIdx.x; }
    // first lane of this environment's half of the wave (EPW == 2), as a ds_bpermute byte address
    const int half_addr_ = EPW > 1 ? (int)(threadIdx.x & (DSIM_NL / EPW)) << 2 : 0;
    // both waves: LDS operations of this wave done, workgroup barrier (no wait for global memory)
    __device__ __forceinline__ void group_barrier() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    static constexpr int NL = DSIM_NL * NW / EPW;
    static constexpr int DSIM_PF = PF;
    // Cross-lane primitives of the wavefront (one wave per environment only): the phase code uses them for the small
    // point-to-point exchanges between lanes that would otherwise be an LDS store, a phase boundary and an LDS load.
    static constexpr bool WAVE_OPS = NW == 1;
    // ... and inside run_wave0 (a phase that only the FIRST wavefront of the environment executes) with any number of waves
    static constexpr bool WAVE0_OPS = true;
    // value of v in lane `src` (any lane): ds_bpermute_b32 -- the LDS crossbar, no LDS memory, no phase boundary.  All
    // lanes of the wave must execute it (uniform control flow); values of lanes that hold nothing meaningful are ignored.
    __device__ __forceinline__ float shfl(float v, int src) {
        return __int_as_float(__builtin_amdgcn_ds_bpermute((src << 2) + half_addr_, __float_as_int(v)));
    }
    // value of v in lane `src`, src uniform across the wave (a compile-time constant after unrolling): v_readlane_b32
    // (two environments per wave: the source differs between the halves -- the crossbar again)
    __device__ __forceinline__ float bcast(float v, int src) {
        if constexpr (EPW > 1) return shfl(v, src);
        else return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
    }
    // value of v in lane + D of the same 16-lane ROW (0 beyond the row's end, 0 from an inactive lane): a DPP row shift on the
    // operand -- VALU latency, no LDS, no SGPR.  Pinned on hardware by tools/micro/dpp_semantics.hip (row_shl:D, bound_ctrl on).
    template <int D> __device__ __forceinline__ float from_above(float v) {
        static_assert(D >= 1 && D <= 15, "row shifts reach 1 .. 15 lanes");
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + D, 0xf, 0xf, true));
    }
    // ... and lane - D of the row (row_shr:D)
    template <int D> __device__ __forceinline__ float from_below(float v) {
        static_assert(D >= 1 && D <= 15, "row shifts reach 1 .. 15 lanes");
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + D, 0xf, 0xf, true));
    }
    // component (P >> 2 c) & 3 of the lane's quad (lanes 4 k .. 4 k + 3) for c = lane & 3: a quad_perm DPP operand.  All four
    // source lanes exist and are active wherever the phase code uses it (uniform control flow).
    template <int P> __device__ __forceinline__ float quad_perm(float v) {
        static_assert(P >= 0 && P <= 0xff, "quad_perm: four two-bit selectors");
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), P, 0xf, 0xf, true));
    }
    // rows 1, 3 of v in rows 0, 2 (v_permlane16_swap: the odd rows of the first operand change places with the even rows of the
    // second; both operands are v) and rows 2, 3 in rows 0, 1 (v_permlane32_swap): the row folds of the quad body level's subtree
    // sums (dsim_core.hpp: dsim_quad_tree_sum).  VALU latency, no LDS; builtins, so the compiler places the hazard waits.  One
    // environment per wavefront only.  Pinned on hardware by tools/micro/dpp_semantics.hip (profiles/quad_adjoint_ab.txt has its output).
    __device__ __forceinline__ float odd_rows(float v) {
        static_assert(EPW == 1, "row folds span the whole wavefront");
        return __int_as_float(__builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false)[1]);
    }
    __device__ __forceinline__ float upper_half(float v) {
        static_assert(EPW == 1, "row folds span the whole wavefront");
        return __int_as_float(__builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false)[1]);
    }
    // a_k += a_k[lane + D of the row] * w for six values at once: v_fmac_f32 with the DPP shift ON ITS OPERAND (the compiler
    // keeps a v_mov_b32_dpp + v_fmac pair for the builtin form: twice the instructions on a path where every issue slot counts).
    // A VGPR written by a VALU instruction may be read through DPP two wait states later at the earliest: the six lines are
    // independent of each other, so only the first needs the s_nop, and a_k's own update is five instructions behind its read.
    // FIRST: the six values may have been written by the instructions right before (the s_nop); later steps of a sum read what
    // the previous step's block wrote five instructions earlier.
    template <int D, bool FIRST = true>
    __device__ __forceinline__ void add_from_above(float& a0, float& a1, float& a2, float& a3, float& a4, float& a5, float w) {
        static_assert(D >= 1 && D <= 15, "row shifts reach 1 .. 15 lanes");
        if constexpr (FIRST) asm volatile("s_nop 1" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5));
        asm volatile("v_fmac_f32_dpp %0, %0, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %1, %1, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %2, %2, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %3, %3, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %4, %4, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %5, %5, %6 row_shl:%7 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5)
                     : "v"(w), "n"(D));
    }
    // every LDS load issued so far has landed: ONE s_waitcnt lgkmcnt(0) behind a batch of loads instead of the partial waits
    // (lgkmcnt(n), n counting down) the compiler otherwise puts in front of each first use.  A lone wave pays a full issue slot
    // (~4.6 cycles, tools/micro/issue_mix.hip) for every s_waitcnt, satisfied or not, while the loads of a batch return a few
    // cycles apart: after the phase's load batch the one full wait is cheaper than a dozen partial ones.
    __device__ __forceinline__ void loads_landed() {
        __builtin_amdgcn_s_waitcnt(0xC07F);   // vmcnt 63, expcnt 7, lgkmcnt 0
    }
    // the same from the NEXT lane of the wave (wave_shl:1: crosses the 16-lane row boundaries; 0 into lane 63)
    template <bool FIRST = true>
    __device__ __forceinline__ void add_from_next(float& a0, float& a1, float& a2, float& a3, float& a4, float& a5, float w) {
        if constexpr (FIRST) asm volatile("s_nop 1" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5));
        asm volatile("v_fmac_f32_dpp %0, %0, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %1, %1, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %2, %2, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %3, %3, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %4, %4, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %5, %5, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5)
                     : "v"(w));
    }
    // ... and from ONE given lane SRC (an edge of the tree that no shift reaches): v_readlane into an SGPR, weighted add
    template <int SRC>
    __device__ __forceinline__ void add_from_lane(float& a0, float& a1, float& a2, float& a3, float& a4, float& a5, float w) {
        const float s0 = bcast(a0, SRC), s1 = bcast(a1, SRC), s2 = bcast(a2, SRC), s3 = bcast(a3, SRC), s4 = bcast(a4, SRC), s5 = bcast(a5, SRC);
        a0 = __builtin_fmaf(s0, w, a0); a1 = __builtin_fmaf(s1, w, a1); a2 = __builtin_fmaf(s2, w, a2);
        a3 = __builtin_fmaf(s3, w, a3); a4 = __builtin_fmaf(s4, w, a4); a5 = __builtin_fmaf(s5, w, a5);
    }
    // this wave's earlier LDS stores are visible to its later LDS loads (DS operations of a wave execute in order)
    __device__ __forceinline__ void lds_fence() { dsim_wave_sync(); }
    // earlier stores to (host-mapped) global memory are visible system-wide before later ones (the model's status words)
    __device__ __forceinline__ void system_fence() { __threadfence_system(); }
    __device__ __forceinline__ void sync() {
        if constexpr (NW == 1) dsim_wave_sync();
        else __syncthreads();
        stamp();
    }
    template <class F> __device__ __forceinline__ void run(F&& f) {
        if (!helper_) f(lane_());
        sync();
    }
    // phase of the first wavefront alone: the link-lane phases of a model whose per-item phases need several wavefronts (row-tree
    // body level of the muscle model).  Inside, the cross-lane primitives above are those of that one wave; side_done() is a no-op
    // (everything the phase reads was finished behind the workgroup barrier in front of it).
    template <class F> __device__ __forceinline__ void run_wave0(F&& f) {
        if constexpr (NW == 1) {
            run(f);
        } else {
            if (threadIdx.x < DSIM_NL) f((int)threadIdx.x);
            sync();
        }
    }
    // phase executed by the helper as well (register-only set-up such as the topology records: each wave keeps its own)
    template <class F> __device__ __forceinline__ void run_both(F&& f) {
        f(lane_());
        sync();
    }
    // fm and fh are two blocks of one phase that touch disjoint LDS words.  With a helper: barrier (everything earlier is
    // visible to both waves), main wave fm / helper wave fh, barrier.  Without: one after the other, as a single wave must.
    template <class FM, class FH> __device__ __forceinline__ void fork_join(FM&& fm, FH&& fh) {
        if constexpr (HELPER) {
            group_barrier();
            if (helper_) fh(lane_());
            else fm(lane_());
            stamp();          // (this wave's block is done; the next stamp is behind the barrier: the difference is waiting)
            group_barrier();
            stamp();
        } else {
            fm(lane_());
            fh(lane_());
            sync();
        }
    }
    // The same with a hand-over INSIDE the main block: fm calls mid() exactly once, at the point from which fh may read what
    // fm has written so far (the kinematics publish poses and twists, then go on with inertias and body forces while the
    // helper evaluates the contacts).  The helper waits at mid()'s barrier instead of at a barrier before the phase; what fm
    // keeps in registers across mid() stays there.  Without a helper: fm, then fh.
    template <class FM, class FH> __device__ __forceinline__ void fork_join_mid(FM&& fm, FH&& fh) {
        if constexpr (HELPER) {
            group_barrier();   // the helper is done with whatever it was left to do beside the previous phase (fork_mid_detached)
            if (helper_) {
                group_barrier();
                fh(lane_());
            } else {
                fm(lane_());
            }
            stamp();
            group_barrier();
            stamp();
        } else {
            fm(lane_());
            fh(lane_());
            sync();
        }
    }
    // ... and with a block fp that the helper runs BEFORE it waits for the hand-over (dsim_core.hpp: dsim_fork_join_mid_pre): fp
    // reads only what was final at the barrier in front of the phase and returns what fh needs of it
    template <class FM, class FP, class FH> __device__ __forceinline__ void fork_join_mid_pre(FM&& fm, FP&& fp, FH&& fh) {
        if constexpr (HELPER) {
            group_barrier();
            if (helper_) {
                const auto pre = fp(lane_());
                stamp();          // (helper: fp is done; the next stamp is behind the hand-over barrier: the difference is waiting)
                group_barrier();
                stamp();
                fh(lane_(), pre);
            } else {
                fm(lane_());
            }
            stamp();
            group_barrier();
            stamp();
        } else {
            fm(lane_());
            fh(lane_(), fp(lane_()));
            sync();
        }
    }
    __device__ __forceinline__ void mid() {
        if constexpr (HELPER || NW > 1) group_barrier();
        else dsim_wave_sync();
        if constexpr (NW > 1) stamp();
    }
    // Several wavefronts per environment (dsim_core.hpp: DsimWideOverlap): f0 is the block of the FIRST wavefront (link lanes, with
    // its cross-lane primitives), fr the block of the others, which sees lanes 0 .. NL - 64 - 1 -- two different instruction
    // streams at the same time.  Where one needs what the other has written both call the same hand-over point -- mid(), mid2(),
    // side_done(): workgroup barriers, so every wavefront must pass each of them exactly once -- and the phase ends with the
    // barrier of sync().  (A branch on the wavefront index is uniform per wave: s_barrier counts waves, not lanes.)
    template <class F0, class FR> __device__ __forceinline__ void fork_wave0(F0&& f0, FR&& fr) {
        static_assert(NW > 1, "fork_wave0 belongs to the mapping with several wavefronts per environment");
        if (threadIdx.x < DSIM_NL) f0((int)threadIdx.x);
        else fr((int)threadIdx.x - DSIM_NL);
        asm volatile("" ::: "memory");
        stamp();
        group_barrier();
        stamp();
    }
    __device__ __forceinline__ void mid2() {
        if constexpr (NW > 1) {
            stamp();   // (developer builds: this wave's arrival; the next stamp is behind the barrier -- the difference is waiting)
            group_barrier();
            stamp();
        }
    }
    // ... and without the barrier at the end: fh is a DETACHED side block -- nothing it reads is written, and nothing it writes is
    // read, before the next barrier that both waves take (the checkpoint copy beside the integrator: the next substep's
    // kinematics start with one).  The main wave goes on at once.
    template <class FM, class FH> __device__ __forceinline__ void fork_mid_detached(FM&& fm, FH&& fh) {
        if constexpr (HELPER) {
            if (helper_) {
                group_barrier();
                fh(lane_());
            } else {
                fm(lane_());
            }
            asm volatile("" ::: "memory");
            stamp();
        } else {
            fm(lane_());
            fh(lane_());
            sync();
        }
    }
    // fh is a side block whose RESULTS fm needs part-way through: fm calls side_done() exactly once, at the point from which it
    // reads what fh wrote (the row-tree body level: the link lanes pick up the per-body contact sums after the first third of
    // their work).  With a helper: the helper runs fh and arrives at the barrier that side_done() is for the main wave; no barrier
    // before (fh must read nothing the main wave wrote since the last barrier both waves took) and none after (the helper is
    // idle until the next fork).  Without: fh, then fm.
    template <class FM, class FH> __device__ __forceinline__ void fork_side(FM&& fm, FH&& fh) {
        if constexpr (HELPER) {
            if (helper_) {
                fh(lane_());
                group_barrier();
            } else {
                fm(lane_());
            }
            asm volatile("" ::: "memory");
            stamp();
        } else {
            fh(lane_());
            dsim_wave_sync();
            fm(lane_());
            sync();
        }
    }
    // (several wavefronts: a no-op inside run_wave0, whose inputs were finished behind the barrier in front of it; the barrier of
    // fork_wave0's first wavefront -- side_done_w())
    __device__ __forceinline__ void side_done() {
        if constexpr (HELPER) group_barrier();
        else if constexpr (NW == 1) dsim_wave_sync();
    }
    __device__ __forceinline__ void side_done_w() {
        stamp();
        group_barrier();
        stamp();
    }
    // phase that only writes global memory nobody in this launch reads back: no vmcnt wait.  One wave: no barrier either
    // (its LDS reads precede, in program order, whatever the next phase stores); several waves: the LDS words it reads
    // must not be overwritten by a wave that runs ahead, hence a barrier.
    template <class F> __device__ __forceinline__ void fire(F&& f) {
        if (!helper_) f(lane_());
        if constexpr (NW > 1) __syncthreads();
    }
    // begin(): the model constants arrive in LDS and the work area is cleared (see DsimImage).  The step functions call it
    // AFTER they have requested their own inputs from global memory (dsim_core.hpp: early loads), so that the launch
    // pays ONE memory latency for all of them instead of one per prologue phase.
    DsimImage<NW, CW, EPW> img_;
    __device__ __forceinline__ void begin_request() {
        if (!helper_) img_.request();
    }
    __device__ __forceinline__ void begin() {
        if (!helper_) img_.land();
        if constexpr (HELPER) group_barrier();
        else sync();
    }
    // per-lane registers of the early loads
    float io_[DSIM_IO_MAX];
    __device__ __forceinline__ float* io(int) { return io_; }
    // Gauss-Jordan inverse of the N x N matrix at H (LDS, row-major), in place, by the first wavefront: lane i holds row i
    // in registers, the pivot row travels through v_readlane (dsim_core.hpp: dsim_fwd_mass has the formulas).
    template <int N> __device__ __forceinline__ void wave_gj(float* H) {
        if constexpr (EPW > 1) dsim_half_gj<N>(H, lane_(), half_addr_);
        else if (!helper_) dsim_wave_gj<N, NW>(H);
        sync();
    }
    // ... of a run-time size n <= NB (generic kernels), padded in registers
    static constexpr bool WAVE_GJ_PAD = EPW == 1;
    template <int NB> __device__ __forceinline__ void wave_gj_pad(float* H, int n) {
        if (!helper_) dsim_wave_gj_pad<NB, NW>(H, n);
        sync();
    }
    // lane-private accumulators of the mass-matrix cotangent (dsim_core.hpp: DSIM_HACC_MAX registers per lane)
    float hacc_[DSIM_HACC_MAX];
    __device__ __forceinline__ float* hacc(int) { return hacc_; }
    float hpf_[DSIM_HPF_MAX];
    __device__ __forceinline__ float* hpf(int) { return hpf_; }
    // per-lane topology records (dsim_core.hpp: DsimTopoRegs, dsim_topo_init)
    DsimTopoRegs topo_;
    __device__ __forceinline__ DsimTopoRegs& topo(int) { return topo_; }
    // per-lane copies of what the joint-space phases would otherwise reload from LDS in every substep (dsim_core.hpp:
    // DsimJointRegs, DsimJointRegsFwd / DsimJointRegsBwd): the dof lane's row of H^-1 and its joint constants.  The flags start
    // false in every launch; kernels whose traits are off never touch the block and it costs them nothing.
    DsimJointRegs jregs_;
    __device__ __forceinline__ DsimJointRegs& jregs(int) { return jregs_; }
    // ... and of what the quad kinematics would reload (dsim_core.hpp: DsimBodyRegs, DsimBodyRegsFwd): the constants of the lane's
    // link and of its chain positions.  Loaded once per forward launch, in front of the substep loop; dead registers elsewhere.
    DsimBodyRegs bregs_;
    __device__ __forceinline__ DsimBodyRegs& bregs(int) { return bregs_; }
    // acc = fma(h[j], x of lane j of this lane's 16-lane ROW, acc) for j = 0 .. N - 1, from acc = 0: the mat-vec of the joint-space
    // phases (dof j on lane j, N <= 16: one row) as N v_fmac_f32 with the broadcast ON THE OPERAND (row_newbcast:j) instead of N
    // v_readlane + v_fmac pairs -- same terms, same order, same fused multiply-add.  x may have been written right before: the
    // s_nop covers the two wait states between a VALU write and a DPP read (as in add_from_above); the accumulator is not read
    // through DPP.  PRECONDITION: every lane of the wave is enabled in EXEC (uniform control flow, as inside Exec::run of the main
    // wave): unlike v_readlane, a DPP operand whose source lane is disabled is not read (bound_ctrl off: the term's write is
    // dropped), so a caller inside a divergent region would get other values than the v_readlane loop.  One environment per
    // wavefront only (the pair kernels keep the crossbar).
    // Pinned on hardware by tools/micro/dpp_semantics.hip (profiles/joint_regs_ab.txt has its output).
    static constexpr bool ROW_BCAST = EPW == 1;
    // ONE asm statement for the whole chain: the compiler puts an s_nop behind every inline-assembly statement, which a statement
    // per term would pay N times.  DSIM_RB_n is the chain of n terms; operand 2 + j is h[j] (h[N - 1] again beyond the model's N).
    // DPP_NEXT: the caller's next use of the result may be a DPP operand (the forward's row shift of qdd to the link lanes).  The
    // compiler's hazard recogniser does not see a VGPR written inside inline assembly, so the two wait states are placed here.
#define DSIM_RB_T(j, op) "v_fmac_f32_dpp %0, %1, %" #op " row_newbcast:" #j " row_mask:0xf bank_mask:0xf\n\t"
#define DSIM_RB_1 DSIM_RB_T(0, 2)
#define DSIM_RB_2 DSIM_RB_1 DSIM_RB_T(1, 3)
#define DSIM_RB_3 DSIM_RB_2 DSIM_RB_T(2, 4)
#define DSIM_RB_4 DSIM_RB_3 DSIM_RB_T(3, 5)
#define DSIM_RB_5 DSIM_RB_4 DSIM_RB_T(4, 6)
#define DSIM_RB_6 DSIM_RB_5 DSIM_RB_T(5, 7)
#define DSIM_RB_7 DSIM_RB_6 DSIM_RB_T(6, 8)
#define DSIM_RB_8 DSIM_RB_7 DSIM_RB_T(7, 9)
#define DSIM_RB_9 DSIM_RB_8 DSIM_RB_T(8, 10)
#define DSIM_RB_10 DSIM_RB_9 DSIM_RB_T(9, 11)
#define DSIM_RB_11 DSIM_RB_10 DSIM_RB_T(10, 12)
#define DSIM_RB_12 DSIM_RB_11 DSIM_RB_T(11, 13)
#define DSIM_RB_13 DSIM_RB_12 DSIM_RB_T(12, 14)
#define DSIM_RB_14 DSIM_RB_13 DSIM_RB_T(13, 15)
#define DSIM_RB_15 DSIM_RB_14 DSIM_RB_T(14, 16)
#define DSIM_RB_16 DSIM_RB_15 DSIM_RB_T(15, 17)
#define DSIM_RB_H(j) "v"(h[(j) < N ? (j) : N - 1])
    // (the accumulator is written by the first term while the later terms still read x and h: early clobber, no input shares its register)
#define DSIM_RB_ASM(n, tail)                                                                                                        \
    asm volatile("s_nop 1\n\t" DSIM_RB_##n tail : "+&v"(acc) : "v"(x), DSIM_RB_H(0), DSIM_RB_H(1), DSIM_RB_H(2), DSIM_RB_H(3),      \
                 DSIM_RB_H(4), DSIM_RB_H(5), DSIM_RB_H(6), DSIM_RB_H(7), DSIM_RB_H(8), DSIM_RB_H(9), DSIM_RB_H(10), DSIM_RB_H(11),   \
                 DSIM_RB_H(12), DSIM_RB_H(13), DSIM_RB_H(14), DSIM_RB_H(15))
#define DSIM_RB_CASE(n)                                                                                                             \
    if constexpr (N == n) {                                                                                                         \
        if constexpr (DPP_NEXT) DSIM_RB_ASM(n, "s_nop 1");                                                                          \
        else DSIM_RB_ASM(n, "");                                                                                                    \
    }
    template <int N, bool DPP_NEXT> __device__ __forceinline__ float row_matvec(const float* h, float x) {
        static_assert(EPW == 1, "the row broadcast serves one environment per wavefront");
        static_assert(N >= 1 && N <= 16, "the dofs must lie in one 16-lane row");
        float acc = 0.f;
        DSIM_RB_CASE(1) DSIM_RB_CASE(2) DSIM_RB_CASE(3) DSIM_RB_CASE(4) DSIM_RB_CASE(5) DSIM_RB_CASE(6) DSIM_RB_CASE(7) DSIM_RB_CASE(8)
        DSIM_RB_CASE(9) DSIM_RB_CASE(10) DSIM_RB_CASE(11) DSIM_RB_CASE(12) DSIM_RB_CASE(13) DSIM_RB_CASE(14) DSIM_RB_CASE(15) DSIM_RB_CASE(16)
        return acc;
    }
#undef DSIM_RB_CASE
#undef DSIM_RB_ASM
#undef DSIM_RB_H
#undef DSIM_RB_16
#undef DSIM_RB_15
#undef DSIM_RB_14
#undef DSIM_RB_13
#undef DSIM_RB_12
#undef DSIM_RB_11
#undef DSIM_RB_10
#undef DSIM_RB_9
#undef DSIM_RB_8
#undef DSIM_RB_7
#undef DSIM_RB_6
#undef DSIM_RB_5
#undef DSIM_RB_4
#undef DSIM_RB_3
#undef DSIM_RB_2
#undef DSIM_RB_1
#undef DSIM_RB_T
    // software prefetch of one checkpoint row: global loads are issued here and stay in flight (registers) until
    // commit() stores them to LDS one adjoint substep later; rows longer than 64*DSIM_PF lanes*regs are read at commit
    // (a native vector type: the may_alias struct dsim_f4 of the copy loops is not promoted to registers -- an array of
    // it ended up in scratch memory with an s_waitcnt vmcnt(0) right behind every prefetch load)
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f pf[DSIM_PF];
    const float* pf_src;
    __device__ __forceinline__ void prefetch(const float* row, int words) {
        pf_src = row;
        if (helper_ || words > 4 * NL * DSIM_PF) return;
        const v4f* r4 = reinterpret_cast<const v4f*>(row);
#pragma unroll
        for (int r = 0; r < DSIM_PF; ++r) {
            const int k = lane_() + NL * r;
            if (4 * k < words) pf[r] = r4[k];
        }
    }
    // ---- the same on the HELPER wavefront (dsim_core.hpp: DsimHelperCommit) ------------------------------------------------
    // both waves: workgroup barrier (the helper waits for the main wave's prologue)
    __device__ __forceinline__ void group_sync() {
        if constexpr (HELPER) group_barrier();
    }
    __device__ __forceinline__ void helper_prefetch(const float* row, int words) {
        if constexpr (HELPER) {
            pf_src = row;
            if (!helper_ || words > 4 * NL * DSIM_PF) return;
            const v4f* r4 = reinterpret_cast<const v4f*>(row);
#pragma unroll
            for (int r = 0; r < DSIM_PF; ++r) {
                const int k = lane_() + NL * r;
                if (4 * k < words) pf[r] = r4[k];
            }
        }
    }
    // helper: the prefetched row -> LDS, then the request for the row after it (next != nullptr); both waves: barrier
    __device__ __forceinline__ void helper_commit(float* dst, int words, const float* next) {
        if constexpr (HELPER) {
            if (helper_) {
                commit(dst, words, lane_());
                if (next) helper_prefetch(next, words);
            }
            asm volatile("" ::: "memory");
            group_barrier();
            stamp();
        }
    }
    // A second block in flight on the helper: the inverse of the mass matrix that the adjoint's first substep needs (fused env
    // adjoint).  Requested at kernel start next to the first row, stored (and its cotangent zeroed) in front of the barrier of the
    // first helper_commit -- the main wave never touches it (Humanoid: 729 words, 12 per lane, that the main wave has no
    // registers to keep in flight across its prologue).  `words`: a multiple of 4, at most 4 * 64 * DSIM_APF.
    static constexpr int DSIM_APF = 4;
    v4f apf[DSIM_APF];
    __device__ __forceinline__ void helper_prefetch_aux(const float* src, int words) {
        if constexpr (HELPER) {
            if (!helper_) return;
            const v4f* s4 = reinterpret_cast<const v4f*>(src);
#pragma unroll
            for (int r = 0; r < DSIM_APF; ++r) {
                const int k = lane_() + NL * r;
                if (4 * k < words) apf[r] = s4[k];
            }
        }
    }
    __device__ __forceinline__ void helper_commit_aux(float* dst, float* zeroed, int words) {
        if constexpr (HELPER) {
            if (!helper_) return;
            v4f *d4 = reinterpret_cast<v4f*>(dst), *z4 = reinterpret_cast<v4f*>(zeroed);
#pragma unroll
            for (int r = 0; r < DSIM_APF; ++r) {
                const int k = lane_() + NL * r;
                if (4 * k < words) {
                    d4[k] = apf[r];
                    z4[k] = v4f{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
    }
    // the same by the wavefronts BEHIND the first one alone (dsim_core.hpp: DsimWideRows; NL - 64 lanes): requested from any phase
    // (the first wavefront returns at once), committed from fork_wave0's second block, which sees lanes 0 .. NL - 64 - 1
    __device__ __forceinline__ void prefetch_rest(const float* row, int words) {
        constexpr int NLR = NL - DSIM_NL;
        pf_src = row;
        if (threadIdx.x < DSIM_NL || words > 4 * NLR * DSIM_PF) return;
        const v4f* r4 = reinterpret_cast<const v4f*>(row);
#pragma unroll
        for (int r = 0; r < DSIM_PF; ++r) {
            const int k = (int)threadIdx.x - DSIM_NL + NLR * r;
            if (4 * k < words) pf[r] = r4[k];
        }
    }
    __device__ __forceinline__ void commit_rest(float* dst, int words, int lane) {
        constexpr int NLR = NL - DSIM_NL;
        if (words > 4 * NLR * DSIM_PF) {
            for (int k = lane; k < words; k += NLR) dst[k] = pf_src[k];
            return;
        }
        v4f* d4 = reinterpret_cast<v4f*>(dst);
#pragma unroll
        for (int r = 0; r < DSIM_PF; ++r) {
            const int k = lane + NLR * r;
            if (4 * k < words) d4[k] = pf[r];
        }
    }
    __device__ __forceinline__ void commit(float* dst, int words, int lane) {
        if (words > 4 * NL * DSIM_PF) {
            for (int k = lane; k < words; k += NL) dst[k] = pf_src[k];
            return;
        }
        v4f* d4 = reinterpret_cast<v4f*>(dst);
#pragma unroll
        for (int r = 0; r < DSIM_PF; ++r) {
            const int k = lane + NL * r;
            if (4 * k < words) d4[k] = pf[r];
        }
    }
};

// Launch modes of the step kernels: 0 one environment per workgroup of NW waves, 1 ... plus its helper wavefront, 2 TWO
// environments per wavefront (DevExec EPW == 2): environment 2 b + h in half h of workgroup b's only wave, LDS images back to back
// Minimum resident waves per SIMD the forward pair kernels are compiled for (0: no constraint).  Ant's env-step pair kernel
// needs 173 VGPRs, five over the 168 of three waves per SIMD: compiled for three it spills those to scratch and the Ant 8192
// rollout drops from 18.4 M to 17.4 M env-steps/s (profiles/r04_pair_ab.txt), so two waves per SIMD (16 environments per CU,
// plain mapping: 12) it is.
#define DSIM_PAIR_WAVES 0
// Kernels with several wavefronts per environment (SNUHumanoid: 4 waves, LDS for two environments per CU) need two resident waves
// per SIMD -- 256 registers per lane, accumulation registers included: one more halves the environments in flight and doubles the
// launch time (measured in round 5: the operator-level adjoint at 257: 0.29 -> 0.53 ms).  The bound makes the compiler keep to it.
// (Not the lean-checkpoint kernels: their adjoint carries the forward phases too and would spill to scratch memory under it.)
#define DSIM_WIDE_WAVES(NW) (((NW) > 1 && !LEAN) ? 2 : 0)
#define DSIM_WAVES_WIDE 4   // wavefronts per environment of those kernels (pick_waves)
#define DSIM_MODE_PLAIN 0
#define DSIM_MODE_HELPER 1
#define DSIM_MODE_PAIR 2
template <class O, class D> struct KCommonT {
    O o;
    D d;
    const uint32_t* cblob;
    float h;
    int substeps, mm_freq, n_envs;
    long long ckpt_stride;  // floats per environment (dsim_ckpt_words)
    // 32-bit words between the constant blocks of two environments: 0 -- ONE block shared by all of them -- or the row length of
    // the model's per-environment block (dsim_model_reserve_env_params), whose row e is then environment e's constants
    long long cblob_stride;
    int* status;            // the model's two status words (host memory mapped into the device): dsim_check_unit_quats
};

// Which step kernels exist: the kernel of direction FWD (a forward kernel) in launch mode MODE, for a model with layout types D
// at NW wavefronts per environment.  Everything that names step kernels -- the launches (dsim_with_flags) and the table of a
// model's kernels (for_each_step_kernel) -- asks here, so the code object holds exactly these.
// HELPER: specialised one-wave kernels of models with ground contacts and without muscles, both directions.  The GENERIC
// one-wave kernels (run-time layout) get a helper wavefront for their ADJOINT only (round 5): its fork_join phases -- the af
// block beside the accumulators of adj H and the per-dof cotangents, contacts^T beside the per-link block of the body level --
// are the same phase code; the generic forward has no split phase, a helper would only idle there.
// PAIR: specialised one-wave models whose phases fit 32 lanes, forward direction only: the adjoint's LDS image (Ant 17 KB) caps
// the environments per CU at the same 8 with either mapping, and a pair wave is 1.26 x as long as a plain one (measured,
// profiles/r04_pair_ab.txt: Ant 8192 adjoint 0.287 ms plain, 0.349 ms pair).
template <class D, int NW, bool FWD, int MODE> constexpr bool dsim_has_mode() {
    if constexpr (MODE == DSIM_MODE_HELPER) {
        if constexpr (std::is_empty<D>::value) return NW == 1 && D::C > 0 && D::NS == 0 && D::L + D::C <= DSIM_NL;
        else return NW == 1 && !FWD;
    } else if constexpr (MODE == DSIM_MODE_PAIR) {
        return FWD && NW == 1 && dsim_pair_ok<D>();
    } else {
        return true;
    }
}
using DsimPlainC = std::integral_constant<int, DSIM_MODE_PLAIN>;
using DsimHelperC = std::integral_constant<int, DSIM_MODE_HELPER>;
using DsimPairC = std::integral_constant<int, DSIM_MODE_PAIR>;
// f(lean, mode) with the two launch-time choices as compile-time constants; a mode whose kernel does not exist for this model
// and direction falls back to the plain kernel (and instantiates nothing).
template <class D, int NW, bool FWD, class F> int dsim_with_flags(bool lean, int mode, F&& f) {
    if constexpr (dsim_has_mode<D, NW, FWD, DSIM_MODE_HELPER>()) {
        if (mode == DSIM_MODE_HELPER) return lean ? f(std::true_type{}, DsimHelperC{}) : f(std::false_type{}, DsimHelperC{});
    }
    if constexpr (dsim_has_mode<D, NW, FWD, DSIM_MODE_PAIR>()) {
        if (mode == DSIM_MODE_PAIR) return lean ? f(std::true_type{}, DsimPairC{}) : f(std::false_type{}, DsimPairC{});
    }
    return lean ? f(std::true_type{}, DsimPlainC{}) : f(std::false_type{}, DsimPlainC{});
}
template <class O> constexpr int dsim_const_words() {
    if constexpr (std::is_empty<O>::value) return O::const_words;
    else return 0;
}
// prefetch registers a model's checkpoint row needs (compile-time layouts), or the generic default of 6 (rows up to 1536 floats
// at one wavefront per environment; longer rows are read at commit time)
template <class O, int NW, bool LEAN, int MODE = 0> constexpr int dsim_pf_regs() {
    if constexpr (std::is_empty<O>::value) {
        // (several wavefronts: rows may be brought in by the wavefronts behind the first one alone, DevExec::prefetch_rest)
        constexpr int words = LEAN ? O::xsc - O::q : O::save_words, lanes = DSIM_NL * (NW > 1 ? NW - 1 : NW) / (MODE == 2 ? 2 : 1);
        return (words / 4 + lanes - 1) / lanes;
    } else {
        return 6;
    }
}
template <int MODE> __device__ __forceinline__ int dsim_env_index() {
    return MODE == DSIM_MODE_PAIR ? 2 * (int)blockIdx.x + (int)(threadIdx.x >> 5) : (int)blockIdx.x;
}
// context of this workgroup's environment; the executor gets the image description and loads it in begin().
// A pair shares ONE copy of the model constants (Ant: 1096 of the forward image's 2332 words; each half loads it, same values
// to the same words, so that a half without an environment -- odd n_envs -- may leave at once): [constants | work 0 | work 1].
// e: the environment, which picks its row of a per-environment constant block (KCommonT::cblob_stride; 0: the one shared block,
// the same address for every e).  The two halves of a pair cannot have rows of their own, so a model in per-environment mode
// never launches the pair kernels (dsim_model::mode) and they keep the unstrided pointer.
template <bool LEAN, int MODE, class Exec, class O, class D>
__device__ __forceinline__ DsimCtxT<O, D, LEAN> start_env(float* lds, const KCommonT<O, D>& k, int image_words, Exec& ex, int e) {
    float* base = MODE == DSIM_MODE_PAIR ? lds + (threadIdx.x >> 5) * (image_words - k.o.const_words) : lds;
    ex.img_.lds = lds;
    ex.img_.work = base;
    if constexpr (MODE == DSIM_MODE_PAIR) ex.img_.cblob = k.cblob;
    else ex.img_.cblob = k.cblob + (long long)e * k.cblob_stride;
    ex.img_.const_words = k.o.const_words;
    ex.img_.image_words = image_words;
    DsimCtxT<O, D, LEAN> c;
    c.s = base;
    c.k = lds;
    c.o = k.o;
    c.d = k.d;
    c.h = k.h;
    return c;
}

template <class O, class D, int NW, bool LEAN, int MODE>
__global__ __launch_bounds__((DSIM_NL * NW * (MODE == 1 ? 2 : 1)), (MODE == DSIM_MODE_PAIR ? DSIM_PAIR_WAVES : DSIM_WIDE_WAVES(NW))) void dsim_fwd_kernel(KCommonT<O, D> k, const float* __restrict__ q_in,
                                                           const float* __restrict__ qd_in,
                                                           const float* __restrict__ act,
                                                           const float* __restrict__ mact, float* q_out,
                                                           float* qd_out, float* ckpt) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = dsim_env_index<MODE>();
    if (e >= k.n_envs) return;
    DevExec<NW, dsim_pf_regs<O, NW, LEAN, MODE>(), dsim_const_words<O>(), MODE == 1, MODE == 2 ? 2 : 1> ex;
    auto c = start_env<LEAN, MODE>(lds, k, k.o.fwd_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd, M = k.d.M;
    dsim_sim_step_forward(c, ex, k.substeps, k.mm_freq, q_in + e * nq, qd_in + e * nd, act + e * nd,
                          M ? mact + e * M : nullptr, q_out + e * nq, qd_out + e * nd,
                          ckpt ? ckpt + (size_t)e * k.ckpt_stride : nullptr, k.status, e);
}

template <class O, class D, int NW, bool LEAN, int MODE>
__global__ __launch_bounds__((DSIM_NL * NW * (MODE == 1 ? 2 : 1)), DSIM_WIDE_WAVES(NW)) void dsim_bwd_kernel(KCommonT<O, D> k, const float* __restrict__ ckpt,
                                                           const float* __restrict__ act,
                                                           const float* __restrict__ mact,
                                                           const float* __restrict__ gq_out,
                                                           const float* __restrict__ gqd_out, float* gq_in,
                                                           float* gqd_in, float* gact, float* gmact, float* lit) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = dsim_env_index<MODE>();
    if (e >= k.n_envs) return;
    DevExec<NW, dsim_pf_regs<O, NW, LEAN, MODE>(), dsim_const_words<O>(), MODE == 1, MODE == 2 ? 2 : 1> ex;
    auto c = start_env<LEAN, MODE>(lds, k, k.o.total_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd, M = k.d.M;
    dsim_sim_step_backward(c, ex, k.substeps, k.mm_freq, ckpt + (size_t)e * k.ckpt_stride, act + e * nd,
                           M ? mact + e * M : nullptr, gq_out + e * nq, gqd_out + e * nd, gq_in + e * nq,
                           gqd_in + e * nd, gact ? gact + e * nd : nullptr, (gmact && M) ? gmact + e * M : nullptr,
                           lit ? lit + (size_t)e * (nq + nd + nd * nd) : nullptr);
}

// dsim_step_backward_multi / dsim_step_jacobian: one workgroup per (environment, cotangent) pair -- the grid is n_envs * n_cot --
// each running the step adjoint above against the environment's checkpoint, which its n_cot sweeps share read-only.  Plain
// launch mode only (the helper-wave kernels compute the same bits); dsim_core.hpp: dsim_multi_slot maps the block index.
template <class O, class D, int NW, bool LEAN>
__global__ __launch_bounds__((DSIM_NL * NW), DSIM_WIDE_WAVES(NW)) void dsim_bwd_multi_kernel(KCommonT<O, D> k, DsimMultiArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if ((long long)blockIdx.x >= (long long)k.n_envs * a.n_cot) return;
    DevExec<NW, dsim_pf_regs<O, NW, LEAN, DSIM_MODE_PLAIN>(), dsim_const_words<O>(), false, 1> ex;
    const DsimMultiSlot s = dsim_multi_slot(a, (int)blockIdx.x, k.d.nd, k.d.M);
    auto c = start_env<LEAN, DSIM_MODE_PLAIN>(lds, k, k.o.total_words, ex, s.env);   // (the constants of the ENVIRONMENT, not of the workgroup)
    dsim_sim_step_backward(c, ex, k.substeps, k.mm_freq, s.ckpt, s.act, s.mact, s.gq_out, s.gqd_out, s.gq_in, s.gqd_in, s.gact,
                           s.gmact);
}

// dsim_step_backward_params: the step adjoint of dsim_bwd_kernel (plain launch mode: the same bits) on the context that switches the
// parameter accumulations on (dsim_core.hpp: DsimParCtxT).  The accumulators are the dsim_par_words(nd, C) LDS words behind the
// adjoint image, which only these kernels are launched with; every output word is written by one lane, environments are not summed.
struct DsimParArgs {
    const float *ckpt, *act, *mact, *gq_out, *gqd_out;
    float *gq_in, *gqd_in, *gact, *gmact;
    float *g_dof, *g_contact;   // [n_envs][5][nd], [n_envs][C][4]; either may be null
};
template <class O, class D, int NW, bool LEAN>
__global__ __launch_bounds__((DSIM_NL * NW), DSIM_WIDE_WAVES(NW)) void dsim_bwd_param_kernel(KCommonT<O, D> k, DsimParArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = (int)blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, dsim_pf_regs<O, NW, LEAN, DSIM_MODE_PLAIN>(), dsim_const_words<O>(), false, 1> ex;
    DsimParCtxT<O, D, LEAN> c;
    static_cast<DsimCtxT<O, D, LEAN>&>(c) = start_env<LEAN, DSIM_MODE_PLAIN>(lds, k, k.o.total_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd, M = k.d.M, C = k.d.C;
    c.pg = lds + k.o.total_words;
    c.g_dof = a.g_dof ? a.g_dof + e * 5 * nd : nullptr;
    c.g_contact = (a.g_contact && C) ? a.g_contact + e * 4 * C : nullptr;
    dsim_sim_step_backward(c, ex, k.substeps, k.mm_freq, a.ckpt + (size_t)e * k.ckpt_stride, a.act + e * nd,
                           M ? a.mact + e * M : nullptr, a.gq_out + e * nq, a.gqd_out + e * nd, a.gq_in + e * nq,
                           a.gqd_in + e * nd, a.gact ? a.gact + e * nd : nullptr, (a.gmact && M) ? a.gmact + e * M : nullptr);
}

// dsim_step_backward_literal, second launch: gq_in[quaternion block of joint j] += rho_j q_j (dsim_literal.hpp).  One thread per
// (environment, link); threads of links without a quaternion joint leave at once.  Run-time layout for every model.
// row_words: floats of one substep's checkpoint row in the model's checkpoint mode (both modes start a row with q, qd).
__global__ __launch_bounds__(64) void dsim_literal_radial_kernel(KCommonT<DsimOff, DsimDims> k, int row_words,
                                                                  const float* __restrict__ ckpt, const float* __restrict__ act,
                                                                  const float* __restrict__ mact, const float* __restrict__ lit,
                                                                  float* gq_in) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x), L = k.d.L;
    const int e = t / L, i = t - e * L;
    if (e >= k.n_envs) return;
    dsim_lit::Consts c;
    c.cb = k.cblob + (long long)e * k.cblob_stride;
    c.o = k.o;
    c.d = k.d;
    const int type = c.I(k.o.jtype, i);
    if (type != DSIM_JOINT_BALL && type != DSIM_JOINT_FREE) return;
    const size_t nq = k.d.nq, nd = k.d.nd, M = k.d.M;
    const float* row = ckpt + (size_t)e * k.ckpt_stride;                  // the first substep's row: (q, qd) as handed in
    const float* hinv = row + (size_t)k.substeps * (size_t)row_words;      // the first group's H^-1
    const float* l = lit + (size_t)e * (nq + nd + nd * nd);
    // (the arrays of a row are padded to 16 bytes each: qd starts at its layout offset, not at nq)
    const float rho = dsim_lit::radial(c, row, row + (k.o.qd - k.o.q), act + e * nd, M ? mact + e * M : nullptr, k.h, hinv, l, l + nq, l + nq + nd, i);
    const int qs = c.I(k.o.qstart, i) + (type == DSIM_JOINT_FREE ? 3 : 0);
    float* g = gq_in + (size_t)e * nq + qs;
    for (int j = 0; j < 4; ++j) g[j] += rho * row[qs + j];
}

template <class O, class D, int NW, bool LEAN, int MODE>
__global__ __launch_bounds__((DSIM_NL * NW * (MODE == 1 ? 2 : 1)), (MODE == DSIM_MODE_PAIR ? DSIM_PAIR_WAVES : DSIM_WIDE_WAVES(NW))) void dsim_env_fwd_kernel(KCommonT<O, D> k, DsimEnvSpec sp, DsimEpisode ep,
                                                               const float* __restrict__ q_in,
                                                               const float* __restrict__ qd_in,
                                                               const float* __restrict__ actions, float* q_out,
                                                               float* qd_out, float* obs, float* rew, float* ckpt) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = dsim_env_index<MODE>();
    if (e >= k.n_envs) return;
    DevExec<NW, dsim_pf_regs<O, NW, LEAN, MODE>(), dsim_const_words<O>(), MODE == 1, MODE == 2 ? 2 : 1> ex;
    auto c = start_env<LEAN, MODE>(lds, k, k.o.fwd_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd;
    dsim_env_fused_forward(c, ex, sp, k.substeps, k.mm_freq, q_in + e * nq, qd_in + e * nd, actions + (size_t)e * sp.n_act,
                           q_out + e * nq, qd_out + e * nd, obs + (size_t)e * sp.n_obs, rew + e,
                           ckpt ? ckpt + (size_t)e * k.ckpt_stride : nullptr, ep, e, k.n_envs, k.status);
}

template <class O, class D, int NW, bool LEAN, int MODE>
__global__ __launch_bounds__((DSIM_NL * NW * (MODE == 1 ? 2 : 1)), DSIM_WIDE_WAVES(NW)) void dsim_env_bwd_kernel(KCommonT<O, D> k, DsimEnvSpec sp,
                                                               const float* __restrict__ ckpt,
                                                               const float* __restrict__ actions,
                                                               const float* __restrict__ gq_out,
                                                               const float* __restrict__ gqd_out,
                                                               const float* __restrict__ gobs,
                                                               const float* __restrict__ grew,
                                                               const float* __restrict__ gobs_before, float* gq_in,
                                                               float* gqd_in, float* gactions) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = dsim_env_index<MODE>();
    if (e >= k.n_envs) return;
    DevExec<NW, dsim_pf_regs<O, NW, LEAN, MODE>(), dsim_const_words<O>(), MODE == 1, MODE == 2 ? 2 : 1> ex;
    auto c = start_env<LEAN, MODE>(lds, k, k.o.total_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd;
    dsim_env_fused_backward(c, ex, sp, k.substeps, k.mm_freq, ckpt + (size_t)e * k.ckpt_stride,
                            actions + (size_t)e * sp.n_act, gq_out ? gq_out + e * nq : nullptr,
                            gqd_out ? gqd_out + e * nd : nullptr, gobs ? gobs + (size_t)e * sp.n_obs : nullptr,
                            grew ? grew + e : nullptr, gobs_before ? gobs_before + (size_t)e * sp.n_obs : nullptr,
                            gq_in + e * nq, gqd_in + e * nd, gactions + (size_t)e * sp.n_act);
}

// dsim_env_step_backward_params: the fused env adjoint of dsim_env_bwd_kernel (plain launch mode: the same bits) on DsimParCtxT,
// as dsim_bwd_param_kernel is the step adjoint on it: the same accumulator words behind the adjoint image, the same outputs.
struct DsimEnvParArgs {
    const float *ckpt, *actions, *gq_out, *gqd_out, *gobs, *grew, *gobs_before;   // cotangent inputs may be null (= zeros)
    float *gq_in, *gqd_in, *gactions;
    float *g_dof, *g_contact;   // [n_envs][5][nd], [n_envs][C][4]; either may be null
};
template <class O, class D, int NW, bool LEAN>
__global__ __launch_bounds__((DSIM_NL * NW), DSIM_WIDE_WAVES(NW)) void dsim_env_bwd_param_kernel(KCommonT<O, D> k, DsimEnvSpec sp, DsimEnvParArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = (int)blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, dsim_pf_regs<O, NW, LEAN, DSIM_MODE_PLAIN>(), dsim_const_words<O>(), false, 1> ex;
    DsimParCtxT<O, D, LEAN> c;
    static_cast<DsimCtxT<O, D, LEAN>&>(c) = start_env<LEAN, DSIM_MODE_PLAIN>(lds, k, k.o.total_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd, C = k.d.C;
    c.pg = lds + k.o.total_words;
    c.g_dof = a.g_dof ? a.g_dof + e * 5 * nd : nullptr;
    c.g_contact = (a.g_contact && C) ? a.g_contact + e * 4 * C : nullptr;
    dsim_env_fused_backward(c, ex, sp, k.substeps, k.mm_freq, a.ckpt + (size_t)e * k.ckpt_stride,
                            a.actions + (size_t)e * sp.n_act, a.gq_out ? a.gq_out + e * nq : nullptr,
                            a.gqd_out ? a.gqd_out + e * nd : nullptr, a.gobs ? a.gobs + (size_t)e * sp.n_obs : nullptr,
                            a.grew ? a.grew + e : nullptr, a.gobs_before ? a.gobs_before + (size_t)e * sp.n_obs : nullptr,
                            a.gq_in + e * nq, a.gqd_in + e * nd, a.gactions + (size_t)e * sp.n_act);
}

template <class O, class D, int NW>
__global__ __launch_bounds__(DSIM_NL * NW) void dsim_env_obs_kernel(KCommonT<O, D> k, DsimEnvSpec sp,
                                                               const float* __restrict__ q,
                                                               const float* __restrict__ qd,
                                                               const float* __restrict__ stored, float* obs,
                                                               float* rew) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = blockIdx.x;
    if (e >= k.n_envs) return;
    DsimCtxT<O, D> c;
    c.s = lds;
    c.k = lds;
    c.o = k.o;
    c.d = k.d;
    c.h = k.h;
    DevExec<NW> ex;
    dsim_env_observe_only(c, ex, sp, q + (size_t)e * k.d.nq, qd + (size_t)e * k.d.nd, stored + (size_t)e * sp.n_act,
                          obs + (size_t)e * sp.n_obs, rew + e);
}

// Differentiable kinematic read-out (dsim_core.hpp: dsim_body_kin_forward / dsim_body_kin_backward): one environment per
// workgroup, plain launch mode.  The forward kernel needs the forward image only; the adjoint re-runs the kinematics phase and
// uses the cotangent arrays of the adjoint image.  dsim_body_transforms is the forward kernel without qd, v_s and status words.
template <class O, class D, int NW>
__global__ __launch_bounds__(DSIM_NL * NW) void dsim_body_kin_kernel(KCommonT<O, D> k, const float* __restrict__ q,
                                                                   const float* __restrict__ qd, float* xsc, float* xsm, float* vs) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, 6, dsim_const_words<O>(), false> ex;
    auto c = start_env<false, DSIM_MODE_PLAIN>(lds, k, k.o.fwd_words, ex, e);
    const size_t L = k.d.L;
    dsim_body_kin_forward(c, ex, q + (size_t)e * k.d.nq, qd ? qd + (size_t)e * k.d.nd : nullptr, xsc + e * 7 * L,
                          xsm ? xsm + e * 7 * L : nullptr, vs ? vs + e * 6 * L : nullptr, k.status, e);
}

template <class O, class D, int NW>
__global__ __launch_bounds__(DSIM_NL * NW) void dsim_body_kin_bwd_kernel(KCommonT<O, D> k, const float* __restrict__ q,
                                                                       const float* __restrict__ qd, const float* __restrict__ gxsc,
                                                                       const float* __restrict__ gxsm, const float* __restrict__ gvs,
                                                                       float* gq, float* gqd) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, 6, dsim_const_words<O>(), false> ex;
    auto c = start_env<false, DSIM_MODE_PLAIN>(lds, k, k.o.total_words, ex, e);
    const size_t L = k.d.L;
    dsim_body_kin_backward(c, ex, q + (size_t)e * k.d.nq, qd ? qd + (size_t)e * k.d.nd : nullptr, gxsc ? gxsc + e * 7 * L : nullptr,
                           gxsm ? gxsm + e * 7 * L : nullptr, gvs ? gvs + e * 6 * L : nullptr, gq + (size_t)e * k.d.nq,
                           gqd ? gqd + (size_t)e * k.d.nd : nullptr);
}


// Differentiable dynamic read-out (dsim_core.hpp: dsim_joint_dyn_forward / dsim_joint_dyn_backward): one environment per
// workgroup, plain launch mode.  The forward kernel needs the forward image only; the adjoint re-runs the forward phases and
// goes on with the mass-matrix and body-level phases of the step adjoint on the adjoint image.
template <class O, class D, int NW>
__global__ __launch_bounds__(DSIM_NL * NW) void dsim_joint_dyn_kernel(KCommonT<O, D> k, const float* __restrict__ q,
                                                                    const float* __restrict__ qd, const float* __restrict__ act,
                                                                    const float* __restrict__ mact, float* tau, float* qdd, float* fs) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, 6, dsim_const_words<O>(), false> ex;
    auto c = start_env<false, DSIM_MODE_PLAIN>(lds, k, k.o.fwd_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd, M = k.d.M, L = k.d.L;
    dsim_joint_dyn_forward(c, ex, q + e * nq, qd + e * nd, act ? act + e * nd : nullptr, (mact && M) ? mact + e * M : nullptr,
                           tau ? tau + e * nd : nullptr, qdd ? qdd + e * nd : nullptr, fs ? fs + e * 6 * L : nullptr, k.status, e);
}

template <class O, class D, int NW>
__global__ __launch_bounds__(DSIM_NL * NW) void dsim_joint_dyn_bwd_kernel(KCommonT<O, D> k, const float* __restrict__ q,
                                                                        const float* __restrict__ qd, const float* __restrict__ act,
                                                                        const float* __restrict__ mact, const float* __restrict__ gtau,
                                                                        const float* __restrict__ gqdd, const float* __restrict__ gfs,
                                                                        float* gq, float* gqd, float* gact, float* gmact) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, 6, dsim_const_words<O>(), false> ex;
    auto c = start_env<false, DSIM_MODE_PLAIN>(lds, k, k.o.total_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd, M = k.d.M, L = k.d.L;
    dsim_joint_dyn_backward(c, ex, q + e * nq, qd + e * nd, act ? act + e * nd : nullptr, (mact && M) ? mact + e * M : nullptr,
                            gtau ? gtau + e * nd : nullptr, gqdd ? gqdd + e * nd : nullptr, gfs ? gfs + e * 6 * L : nullptr,
                            gq + e * nq, gqd + e * nd, gact ? gact + e * nd : nullptr, (gmact && M) ? gmact + e * M : nullptr);
}

// Differentiable ground-contact read-out (dsim_core.hpp: dsim_ground_contact_forward / dsim_ground_contact_backward): one
// environment per workgroup, plain launch mode.  The forward kernel needs the forward image only; the adjoint re-runs the
// kinematics phase and uses the cotangent arrays of the adjoint image.
template <class O, class D, int NW>
__global__ __launch_bounds__(DSIM_NL * NW) void dsim_ground_con_kernel(KCommonT<O, D> k, const float* __restrict__ q,
                                                                     const float* __restrict__ qd, float* point, float* vel,
                                                                     float* force, float* lw) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, 6, dsim_const_words<O>(), false> ex;
    auto c = start_env<false, DSIM_MODE_PLAIN>(lds, k, k.o.fwd_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd, C = k.d.C, L = k.d.L;
    dsim_ground_contact_forward(c, ex, q + e * nq, qd + e * nd, point ? point + e * 3 * C : nullptr, vel ? vel + e * 3 * C : nullptr,
                                force ? force + e * 3 * C : nullptr, lw ? lw + e * 6 * L : nullptr, k.status, e);
}

template <class O, class D, int NW>
__global__ __launch_bounds__(DSIM_NL * NW) void dsim_ground_con_bwd_kernel(KCommonT<O, D> k, const float* __restrict__ q,
                                                                         const float* __restrict__ qd, const float* __restrict__ gpoint,
                                                                         const float* __restrict__ gvel, const float* __restrict__ gforce,
                                                                         const float* __restrict__ glw, float* gq, float* gqd) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, 6, dsim_const_words<O>(), false> ex;
    auto c = start_env<false, DSIM_MODE_PLAIN>(lds, k, k.o.total_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd, C = k.d.C, L = k.d.L;
    dsim_ground_contact_backward(c, ex, q + e * nq, qd + e * nd, gpoint ? gpoint + e * 3 * C : nullptr,
                                 gvel ? gvel + e * 3 * C : nullptr, gforce ? gforce + e * 3 * C : nullptr,
                                 glw ? glw + e * 6 * L : nullptr, gq + e * nq, gqd + e * nd);
}


// Differentiable mass matrix read-out (dsim_core.hpp: dsim_mass_forward / dsim_mass_backward): one environment per workgroup,
// plain launch mode.  The forward kernel needs the forward image only; the adjoint re-runs the forward phases and goes on with
// the mass-matrix and body-level phases of the step adjoint on the adjoint image.
template <class O, class D, int NW>
__global__ __launch_bounds__(DSIM_NL * NW) void dsim_mass_kernel(KCommonT<O, D> k, const float* __restrict__ q, float* H,
                                                               float* Hinv, float* S) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, 6, dsim_const_words<O>(), false> ex;
    auto c = start_env<false, DSIM_MODE_PLAIN>(lds, k, k.o.fwd_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd;
    dsim_mass_forward(c, ex, q + e * nq, H ? H + e * nd * nd : nullptr, Hinv ? Hinv + e * nd * nd : nullptr,
                      S ? S + e * 6 * nd : nullptr, k.status, e);
}

template <class O, class D, int NW>
__global__ __launch_bounds__(DSIM_NL * NW) void dsim_mass_bwd_kernel(KCommonT<O, D> k, const float* __restrict__ q,
                                                                   const float* __restrict__ gH, const float* __restrict__ gHinv,
                                                                   const float* __restrict__ gS, float* gq) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int e = blockIdx.x;
    if (e >= k.n_envs) return;
    DevExec<NW, 6, dsim_const_words<O>(), false> ex;
    auto c = start_env<false, DSIM_MODE_PLAIN>(lds, k, k.o.total_words, ex, e);
    const size_t nq = k.d.nq, nd = k.d.nd;
    dsim_mass_backward(c, ex, q + e * nq, gH ? gH + e * nd * nd : nullptr, gHinv ? gHinv + e * nd * nd : nullptr,
                       gS ? gS + e * 6 * nd : nullptr, gq + e * nq);
}


// The per-environment constant block (dsim_model_reserve_env_params): [rows][row_words] 32-bit words, row_words a multiple of 4 and
// every row 16-byte aligned, as DsimImage fetches it.
// Fill: row blockIdx.x <- the shared block, 16 bytes per lane and copy.
__global__ __launch_bounds__(64) void dsim_env_params_fill_kernel(const uint32_t* __restrict__ shared, uint32_t* rows, int row_words,
                                                                   int n_rows) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    const int r = (int)blockIdx.x;
    if (r >= n_rows) return;
    const v4f* src = reinterpret_cast<const v4f*>(shared);
    v4f* dst = reinterpret_cast<v4f*>(rows + (size_t)r * (size_t)row_words);
    for (int i = (int)threadIdx.x; i < row_words / 4; i += (int)blockDim.x) dst[i] = src[i];
}
// Scatter: words [off, off + n) of row r <- values[r * src_stride + (0 .. n - 1)] for r < n_rows; src_stride 0 broadcasts one
// array into every row (dsim_model_set_params in per-environment mode).  blocks_per_row workgroups of 64 lanes per row,
// consecutive lanes on consecutive words of it.
__global__ __launch_bounds__(64) void dsim_env_params_scatter_kernel(const float* __restrict__ values, long long src_stride,
                                                                      uint32_t* rows, int row_words, int off, int n, int n_rows,
                                                                      int blocks_per_row) {
    const int r = (int)(blockIdx.x / (unsigned)blocks_per_row);
    const int j = (int)(blockIdx.x - (unsigned)r * (unsigned)blocks_per_row) * 64 + (int)threadIdx.x;
    if (r >= n_rows || j >= n) return;
    reinterpret_cast<float*>(rows)[(size_t)r * (size_t)row_words + (size_t)(off + j)] = values[(size_t)r * (size_t)src_stride + (size_t)j];
}

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return DSIM_ERR_HIP;
}

// ---- kernel variants -------------------------------------------------------------------------------
enum Variant {
    V_GENERIC = 0,
#define DSIM_ENUM(T) V_##T,
    DSIM_STATIC_VARIANTS(DSIM_ENUM)
#undef DSIM_ENUM
};

int match_variant(const DsimLayout& lay) {
    if (getenv("DSIM_FORCE_GENERIC")) return V_GENERIC;
    const size_t no = sizeof(DsimOff) / sizeof(int), nd = sizeof(DsimDims) / sizeof(int);
#define DSIM_MATCH(T)                                                                                              \
    if (sizeof(kDsimStatic##T) == (no + nd) * sizeof(int) && memcmp(kDsimStatic##T, &lay.o, no * sizeof(int)) == 0 && \
        memcmp(kDsimStatic##T + no, &lay.d, nd * sizeof(int)) == 0)                                                 \
        return V_##T;
    DSIM_STATIC_VARIANTS(DSIM_MATCH)
#undef DSIM_MATCH
    return V_GENERIC;
}

}  // namespace

struct dsim_model {
    DsimLayout lay;
    uint32_t* d_cblob = nullptr;
    float* d_eye = nullptr;   // (n_q + n_qd)-square identity: the seed rows of dsim_step_jacobian
    // Per-environment mode (dsim_model_reserve_env_params): env_rows > 0 rows of env_words() words, row e the constant block of
    // environment e; every launch then reads d_env_cblob with that stride instead of d_cblob (make_k).  d_cblob stays what
    // dsim_model_set_params last wrote: the values "for all environments" that a new reservation starts from.
    uint32_t* d_env_cblob = nullptr;
    int env_rows = 0;
    int env_words() const { return ((int)lay.cblob.size() + 3) & ~3; }
    int variant = V_GENERIC;
    int waves = 1;   // wavefronts per environment: 1 or DSIM_WAVES_WIDE
    int lean = 0;    // checkpoint mode (dsim_model_set_ckpt_mode)
    int device = 0;  // HIP device the constants live on (the current device of dsim_model_create); every call checks it
    // Status words written by the kernels (dsim_core.hpp: dsim_check_unit_quats): [0] != 0 -- a launch was handed a non-unit
    // quaternion, [1] -- the environment that saw it.  Pinned host memory mapped into the device: a kernel's store lands here
    // without any copy, and the next call on the model reads it without touching the stream (no synchronisation anywhere).
    volatile int* h_status = nullptr;
    int* d_status = nullptr;
    int row_words() const { return lean ? lay.o.xsc - lay.o.q : lay.o.save_words; }
    // Helper-wave kernels (DevExec<..., HELPER>) are used while every environment of the launch is resident at once: the
    // helper takes a wave slot of its SIMD, so beyond that point (several rounds of workgroups) it would halve the
    // number of environments in flight -- measured: Ant 8192 envs 13.4 M env-steps/s without, 8.1 M with.
    int helper_max_envs = 0;
    bool helper_ok(int n_envs) const { return n_envs <= helper_max_envs; }
    // Two environments per wavefront (DSIM_MODE_PAIR; forward kernels of models with pair kernels only -- dsim_with_flags falls
    // back to the plain kernels for the others): every launch beyond the helper-wave capacity.  A pair wave is a few per cent
    // longer than a plain one (items beyond 32 lanes take two passes) and carries two environments: half the waves per launch,
    // and a third more environments resident per CU (Ant: 16 instead of 12).  DSIM_PAIR=0 / 1 forces the choice (A/B runs).
    int pair_min_envs = 1 << 30;
    // (never in per-environment mode: a pair shares ONE copy of the constants between its two environments -- start_env)
    int mode(int n_envs, bool fwd) const {
        if (helper_ok(n_envs)) return DSIM_MODE_HELPER;
        if (!fwd || env_rows) return DSIM_MODE_PLAIN;
        return n_envs >= pair_min_envs ? DSIM_MODE_PAIR : DSIM_MODE_PLAIN;
    }
};
void dsim_helper_capacity(dsim_model* m);

namespace {

// calls f(offsets, dims, waves) with the (static or runtime) layout types of the model's kernel variant and the number of
// wavefronts per environment as a compile-time constant
template <class D> constexpr bool dsim_static_wide() { return D::NS > DSIM_NL || D::C > DSIM_NL; }
template <class F> int dispatch(const dsim_model* m, F&& f) {
    const bool wide = m->waves > 1;
    switch (m->variant) {
    // a specialised variant exists with the wave count its model wants (pick_waves), not with both
#define DSIM_CASE(T)                                                                                        \
    case V_##T:                                                                                             \
        if constexpr (dsim_static_wide<DsimDims##T>())                                                      \
            return f(DsimOff##T{}, DsimDims##T{}, std::integral_constant<int, DSIM_WAVES_WIDE>{});          \
        else                                                                                                \
            return f(DsimOff##T{}, DsimDims##T{}, std::integral_constant<int, 1>{});
        DSIM_STATIC_VARIANTS(DSIM_CASE)
#undef DSIM_CASE
        default:
            return wide ? f(m->lay.o, m->lay.d, std::integral_constant<int, DSIM_WAVES_WIDE>{})
                        : f(m->lay.o, m->lay.d, std::integral_constant<int, 1>{});
    }
}

// Wavefronts per environment.  One wave is the lowest-latency mapping while the per-item phases are one or two passes
// over a wavefront (Ant, Humanoid, the planar models, cartpole): a workgroup barrier costs more than a second pass, and
// 4 waves per environment need 4 resident waves per SIMD at 1024 environments, which the kernels' ~200 registers per
// lane do not allow (measured: Humanoid forward 0.45 -> 0.90 ms).  Models with item lists several wavefronts long
// (SNUHumanoid: 198 muscle segments, 88 contacts) run 4 waves per environment: their long phases become single
// passes on the CU's 4 SIMDs (SNUHumanoid 512 envs: 0.62 + 0.98 -> 0.45 + 0.62 ms).  DSIM_WAVES=1|4 overrides the
// choice for the generic kernels (A/B runs: DSIM_FORCE_GENERIC=1 DSIM_WAVES=...).
int pick_waves(const DsimLayout& lay, int variant) {
    const DsimDims& d = lay.d;
    const int want = (d.NS > DSIM_NL || d.C > DSIM_NL) ? DSIM_WAVES_WIDE : 1;
    if (variant != V_GENERIC) return want;   // specialised kernels are compiled for their model's wave count only
    if (const char* e = getenv("DSIM_WAVES")) return atoi(e) > 1 ? DSIM_WAVES_WIDE : 1;
    return want;
}

template <class O, class D>
KCommonT<O, D> make_k(const dsim_model* m, O o, D d, int n_envs, float dt, int substeps, int mm_freq) {
    KCommonT<O, D> k;
    k.o = o;
    k.d = d;
    k.cblob = m->env_rows ? m->d_env_cblob : m->d_cblob;
    k.cblob_stride = m->env_rows ? m->env_words() : 0;
    k.h = dt / float(substeps);
    k.substeps = substeps;
    k.mm_freq = mm_freq;
    k.n_envs = n_envs;
    k.ckpt_stride = dsim_ckpt_words(m->row_words(), m->lay.d.nq, m->lay.d.nd, substeps, mm_freq);
    k.status = m->d_status;
    return k;
}

// a model belongs to the device it was created on: its constant block lives there and the kernel attributes / occupancy
// figures were set up for it.  One process may drive several GPUs (one model per GPU); a call must run with its model's
// device current, and the stream and pointers it is given must belong to that device.
int check_device(const dsim_model* m) {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    if (dev != m->device)
        return fail(DSIM_ERR_INVALID, "model was created on HIP device " + std::to_string(m->device) + " but the current device is " +
                                          std::to_string(dev) + " (hipSetDevice / torch.cuda.device before the call)");
    return DSIM_OK;
}

// A launch that was handed a non-unit quaternion leaves a mark in the model's status words; the next call that would launch
// on the model reports it (once: the mark is cleared) instead of launching.  Asynchronous, like a HIP error of a kernel:
// the state the marked launch returned is what the formulas give off the manifold, not what the reference gives there.
int check_status(const dsim_model* m) {
    if (m->h_status && m->h_status[0] != 0) {
        const int env = m->h_status[1];
        m->h_status[0] = 0;
        return fail(DSIM_ERR_INVALID, "an earlier launch on this model was given a joint_q whose quaternion block is not a unit "
                                      "quaternion (| |q| - 1 | > 1e-4; first seen in environment " + std::to_string(env) +
                                          "): the path is defined on unit quaternions only (include/dsim.h, dsim_step_forward); "
                                          "normalise the state before handing it in");
    }
    return DSIM_OK;
}

int check_common(const dsim_model* m, int n_envs, float dt, int substeps, int mm_freq) {
    if (!m) return fail(DSIM_ERR_INVALID, "null model");
    if (int rc = check_device(m)) return rc;
    if (int rc = check_status(m)) return rc;
    if (n_envs <= 0) return fail(DSIM_ERR_INVALID, "n_envs must be positive");
    if (m->env_rows && n_envs > m->env_rows)
        return fail(DSIM_ERR_INVALID, "n_envs = " + std::to_string(n_envs) + " but the model holds per-environment parameters for " +
                                          std::to_string(m->env_rows) + " environments (dsim_model_reserve_env_params)");
    if (substeps <= 0 || mm_freq <= 0) return fail(DSIM_ERR_INVALID, "substeps and mm_freq must be positive");
    if (!(dt > 0.f)) return fail(DSIM_ERR_INVALID, "dt must be positive");
    return DSIM_OK;
}

int launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return DSIM_OK;
}

// The four families of step kernels (a function template cannot be a template argument; a family names its kernels).
#define DSIM_STEP_FAMILY(NAME, IS_FWD)                                                      \
    struct NAME##_family {                                                                  \
        static constexpr bool FWD = IS_FWD;                                                 \
        static constexpr const char* what = "launch " #NAME;                                \
        template <class O, class D, int NW, bool LEAN, int MODE> static constexpr auto kernel() { return &NAME<O, D, NW, LEAN, MODE>; } \
    };
DSIM_STEP_FAMILY(dsim_bwd_kernel, false)
DSIM_STEP_FAMILY(dsim_env_bwd_kernel, false)
DSIM_STEP_FAMILY(dsim_fwd_kernel, true)
DSIM_STEP_FAMILY(dsim_env_fwd_kernel, true)
#undef DSIM_STEP_FAMILY

// f(kernel, is_forward, lean, mode) for every step kernel of a model: operator and env step, forward and adjoint, full and lean
// checkpoints, every launch mode in which the kernel exists (dsim_has_mode).
template <class O, class D, int NW, class F> void for_each_step_kernel(F&& f) {
    auto one = [&](auto fam, auto lean_c, auto mode_c) {
        using Fam = decltype(fam);
        constexpr bool LEAN = decltype(lean_c)::value;
        constexpr int MODE = decltype(mode_c)::value;
        if constexpr (dsim_has_mode<D, NW, Fam::FWD, MODE>())
            f(reinterpret_cast<const void*>(Fam::template kernel<O, D, NW, LEAN, MODE>()), Fam::FWD, LEAN, MODE);
    };
    auto mode = [&](auto mode_c) {
        auto lean = [&](auto lean_c) {
            one(dsim_bwd_kernel_family{}, lean_c, mode_c);
            one(dsim_env_bwd_kernel_family{}, lean_c, mode_c);
            one(dsim_fwd_kernel_family{}, lean_c, mode_c);
            one(dsim_env_fwd_kernel_family{}, lean_c, mode_c);
        };
        lean(std::false_type{});
        lean(std::true_type{});
    };
    mode(DsimPlainC{});
    mode(DsimHelperC{});
    mode(DsimPairC{});
}

// The one launch site of the step kernels: kernel variant, wave count, checkpoint mode and launch mode become compile-time
// constants, and the geometry follows from them -- EPB environments per workgroup (2 in pair mode), one workgroup of NW waves
// (+ the helper wave) each, and the LDS image(s) of the direction (a pair shares one copy of the model constants: start_env).
// `args`: the kernel's arguments behind its KCommonT.
template <class Fam, class... Args>
int launch_step(const dsim_model* m, int n_envs, float dt, int substeps, int mm_freq, void* hip_stream, Args... args) {
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return dispatch(m, [&](auto o, auto d, auto nw) {
        using O = decltype(o);
        using D = decltype(d);
        constexpr int NW = decltype(nw)::value;
        auto k = make_k(m, o, d, n_envs, dt, substeps, mm_freq);
        const size_t image_words = Fam::FWD ? m->lay.o.fwd_words : m->lay.o.total_words, const_words = m->lay.o.const_words;
        dsim_with_flags<D, NW, Fam::FWD>(m->lean, m->mode(n_envs, Fam::FWD), [&](auto lean_c, auto mode_c) {
            constexpr bool LEAN = decltype(lean_c)::value;
            constexpr int MODE = decltype(mode_c)::value, EPB = MODE == DSIM_MODE_PAIR ? 2 : 1;
            hipLaunchKernelGGL((Fam::template kernel<O, D, NW, LEAN, MODE>()), dim3((n_envs + EPB - 1) / EPB),
                               dim3(DSIM_NL * NW * (MODE == DSIM_MODE_HELPER ? 2 : 1)),
                               (image_words * EPB - const_words * (EPB - 1)) * 4, st, k, args...);
            return 0;
        });
        return launched(Fam::what);
    });
}

// The read-out kernels: one environment per workgroup of NW waves, plain launch mode, no step geometry.  A family names the
// kernel, the LDS image it runs on (FWD: the forward image, otherwise the adjoint image) and whether the launch enforces the
// unit-quaternion precondition (CHECKS: the kernel gets the model's status words; otherwise none -- a read-back of whatever state
// the caller holds, or an adjoint whose forward launch checked the state).
#define DSIM_READOUT_FAMILY(NAME, IS_FWD, DOES_CHECK)                                                  \
    struct NAME##_family {                                                                             \
        static constexpr bool FWD = IS_FWD, CHECKS = DOES_CHECK;                                       \
        static constexpr const char* what = "launch " #NAME;                                           \
        template <class O, class D, int NW> static constexpr auto kernel() { return &NAME<O, D, NW>; } \
    };
DSIM_READOUT_FAMILY(dsim_env_obs_kernel, true, true)
DSIM_READOUT_FAMILY(dsim_body_kin_kernel, true, true)
DSIM_READOUT_FAMILY(dsim_body_kin_bwd_kernel, false, false)
DSIM_READOUT_FAMILY(dsim_joint_dyn_kernel, true, true)
DSIM_READOUT_FAMILY(dsim_joint_dyn_bwd_kernel, false, false)
DSIM_READOUT_FAMILY(dsim_ground_con_kernel, true, true)
DSIM_READOUT_FAMILY(dsim_ground_con_bwd_kernel, false, false)
DSIM_READOUT_FAMILY(dsim_mass_kernel, true, true)
DSIM_READOUT_FAMILY(dsim_mass_bwd_kernel, false, false)
#undef DSIM_READOUT_FAMILY
// dsim_body_transforms: the kinematic read-out without qd and v_s, and without the precondition
struct dsim_body_xf_family : dsim_body_kin_kernel_family {
    static constexpr bool CHECKS = false;
};
// The list of the read-out families: the table below walks it, and launch_readout refuses to compile for a family that is not
// on it (or derived from one that is), so a kernel cannot be launched without being opted in to its LDS size.
using dsim_readout_families = std::tuple<dsim_env_obs_kernel_family, dsim_body_kin_kernel_family, dsim_body_kin_bwd_kernel_family,
                                         dsim_joint_dyn_kernel_family, dsim_joint_dyn_bwd_kernel_family,
                                         dsim_ground_con_kernel_family, dsim_ground_con_bwd_kernel_family,
                                         dsim_mass_kernel_family, dsim_mass_bwd_kernel_family>;
template <class Fam, class... Listed> constexpr bool dsim_readout_listed(std::tuple<Listed...>*) {
    return (std::is_base_of<Listed, Fam>::value || ...);
}

// f(kernel) for every kernel of a model outside the step families: the read-outs above, the multi-cotangent sweep and the
// parameter-gradient sweeps of the step and of the fused env step (full and lean checkpoints; step_backward_multi,
// dsim_step_backward_params and dsim_env_step_backward_params launch them).
template <class O, class D, int NW, class F, class... Listed> void for_each_readout_kernel(F&& f, std::tuple<Listed...>*) {
    (f(reinterpret_cast<const void*>(Listed::template kernel<O, D, NW>())), ...);
    f(reinterpret_cast<const void*>(&dsim_bwd_multi_kernel<O, D, NW, false>));
    f(reinterpret_cast<const void*>(&dsim_bwd_multi_kernel<O, D, NW, true>));
    f(reinterpret_cast<const void*>(&dsim_bwd_param_kernel<O, D, NW, false>));
    f(reinterpret_cast<const void*>(&dsim_bwd_param_kernel<O, D, NW, true>));
    f(reinterpret_cast<const void*>(&dsim_env_bwd_param_kernel<O, D, NW, false>));
    f(reinterpret_cast<const void*>(&dsim_env_bwd_param_kernel<O, D, NW, true>));
}
template <class O, class D, int NW, class F> void for_each_readout_kernel(F&& f) {
    for_each_readout_kernel<O, D, NW>(f, static_cast<dsim_readout_families*>(nullptr));
}

// The one launch site of the read-out kernels.  `args`: the kernel's arguments behind its KCommonT.
template <class Fam, class... Args> int launch_readout(const dsim_model* m, int n_envs, void* hip_stream, Args... args) {
    static_assert(dsim_readout_listed<Fam>(static_cast<dsim_readout_families*>(nullptr)), "add the family to dsim_readout_families");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return dispatch(m, [&](auto o, auto d, auto nw) {
        constexpr int NW = decltype(nw)::value;
        auto k = make_k(m, o, d, n_envs, 1.0f, 1, 1);
        if (!Fam::CHECKS) k.status = nullptr;
        hipLaunchKernelGGL((Fam::template kernel<decltype(o), decltype(d), NW>()), dim3(n_envs), dim3(DSIM_NL * NW),
                           (size_t)(Fam::FWD ? m->lay.o.fwd_words : m->lay.o.total_words) * 4, st, k, args...);
        return launched(Fam::what);
    });
}

// the model's device / host allocations and the model itself (a model whose creation failed half-way included)
void free_model(dsim_model* m) {
    if (m->d_cblob) (void)hipFree(m->d_cblob);
    if (m->d_env_cblob) (void)hipFree(m->d_env_cblob);
    if (m->d_eye) (void)hipFree(m->d_eye);
    if (m->h_status) (void)hipHostFree(const_cast<int*>(m->h_status));
    delete m;
}

int make_spec(const dsim_model* m, const dsim_env_spec* e, DsimEnvSpec& sp) {
    if (!e) return fail(DSIM_ERR_INVALID, "null env spec");
    const DsimDims& d = m->lay.d;
    if (e->kind != DSIM_ENV_LOCOMOTION && e->kind != DSIM_ENV_CARTPOLE && e->kind != DSIM_ENV_PLANAR)
        return fail(DSIM_ERR_INVALID, "unknown env kind");
    if (e->n_act <= 0 || e->n_act > (d.M > d.nd ? d.M : d.nd)) return fail(DSIM_ERR_INVALID, "n_act out of range");
    if (!e->act_scale) return fail(DSIM_ERR_INVALID, "null act_scale");
    if (e->act_muscle) {
        if (e->n_act != d.M) return fail(DSIM_ERR_INVALID, "muscle actions must match the muscle count");
    } else if (e->act_offset < 0 || e->act_offset + e->n_act > d.nd) {
        return fail(DSIM_ERR_INVALID, "action dofs out of range");
    }
    int expect;
    if (e->kind == DSIM_ENV_LOCOMOTION) {
        if (d.nq < 7 || d.nd < 6 || m->lay.cblob[m->lay.o.jtype] != DSIM_JOINT_FREE)
            return fail(DSIM_ERR_INVALID, "locomotion observations need a free-floating root joint");
        expect = 13 + (d.nq - 7) + (d.nd - 6) + (e->obs_actions ? e->n_act : 0);
    } else if (e->kind == DSIM_ENV_PLANAR) {
        if (d.nq != d.nd || d.nq < 3) return fail(DSIM_ERR_INVALID, "planar observations need a 3-dof planar root");
        expect = d.nq - 1 + d.nd;
    } else {
        if (d.nq != 2 || d.nd != 2) return fail(DSIM_ERR_INVALID, "cartpole observations need 2 coordinates");
        expect = 5;
    }
    if (e->n_obs != expect) return fail(DSIM_ERR_INVALID, "n_obs does not match the observation layout");
    sp = dsim_env_spec_copy(*e);
    return DSIM_OK;
}

}  // namespace

extern "C" {

const char* dsim_last_error(void) { return g_err.c_str(); }
int dsim_version(void) { return 110; }

int dsim_model_create(const dsim_model_desc* desc, dsim_model** out) {
    if (!desc || !out) return fail(DSIM_ERR_INVALID, "null argument");
    dsim_model* m = new (std::nothrow) dsim_model();
    if (!m) return fail(DSIM_ERR_INVALID, "out of host memory");
    std::string err = dsim_build_layout(*desc, m->lay);
    if (!err.empty()) {
        delete m;
        return fail(DSIM_ERR_INVALID, err);
    }
    const int bytes = m->lay.o.total_words * 4, fbytes = m->lay.o.fwd_words * 4;
    if (bytes > 160 * 1024) {
        delete m;
        return fail(DSIM_ERR_LIMIT, "model needs more than 160 KiB of LDS per environment");
    }
    m->variant = match_variant(m->lay);
    m->waves = pick_waves(m->lay, m->variant);
    hipError_t e = hipGetDevice(&m->device);
    if (e == hipSuccess) {
        void* hp = nullptr;
        e = hipHostMalloc(&hp, 2 * sizeof(int), hipHostMallocMapped);
        if (e == hipSuccess) {
            m->h_status = static_cast<volatile int*>(hp);
            m->h_status[0] = m->h_status[1] = 0;
            void* dp = nullptr;
            e = hipHostGetDevicePointer(&dp, hp, 0);
            m->d_status = static_cast<int*>(dp);
        }
    }
    if (e == hipSuccess) e = hipMalloc(&m->d_cblob, sizeof(uint32_t) * m->lay.cblob.size());
    if (e == hipSuccess)
        e = hipMemcpy(m->d_cblob, m->lay.cblob.data(), sizeof(uint32_t) * m->lay.cblob.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const size_t K = (size_t)m->lay.d.nq + (size_t)m->lay.d.nd;
        std::string eye(K * K * sizeof(float), '\0');
        float* h_eye = reinterpret_cast<float*>(&eye[0]);
        for (size_t i = 0; i < K; ++i) h_eye[i * K + i] = 1.0f;
        e = hipMalloc(&m->d_eye, eye.size());
        if (e == hipSuccess) e = hipMemcpy(m->d_eye, h_eye, eye.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && (2 * bytes > 64 * 1024 || 2 * fbytes > 64 * 1024)) {   // (2 x: pair launches)
        // Opt in to > 64 KiB of dynamic LDS.  The attribute belongs to the kernel FUNCTION, not to this model: two models
        // that share a kernel variant (e.g. two user models on the generic kernels) must not lower each other's limit,
        // so it is set once to the hardware maximum (160 KiB); what a launch actually gets is its own byte count.
        dispatch(m, [&](auto o, auto d, auto nw) {
            using O = decltype(o);
            using D = decltype(d);
            constexpr int NW = decltype(nw)::value;
            auto opt_in = [&](const void* fn) {
                if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            };
            for_each_step_kernel<O, D, NW>([&](const void* fn, bool, bool, int) { opt_in(fn); });
            for_each_readout_kernel<O, D, NW>(opt_in);
            return 0;
        });
    }
    if (e != hipSuccess) {
        free_model(m);
        return hip_fail(e, "dsim_model_create");
    }
    dsim_helper_capacity(m);
    *out = m;
    return DSIM_OK;
}

}  // extern "C"

// helper-wave kernels: how many environments are resident at once (the smallest figure over the model's kernels in the
// current checkpoint mode); DSIM_HELPER=0 / 1 forces the choice (A/B runs)
void dsim_helper_capacity(dsim_model* m) {
    dispatch(m, [&](auto o, auto d, auto nw) {
        using O = decltype(o);
        using D = decltype(d);
        constexpr int NW = decltype(nw)::value;
        if constexpr (dsim_has_mode<D, NW, false, DSIM_MODE_HELPER>()) {
            int cus = 0, per_cu = 1 << 20;   // (callers have the model's device current: dsim_model_create, check_device)
            bool ok = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device) == hipSuccess;
            // resident workgroups per CU of each helper kernel (the lean ones count once the model is in that mode: it is chosen
            // right after creation, and dsim_model_set_ckpt_mode re-evaluates)
            for_each_step_kernel<O, D, NW>([&](const void* fn, bool fwd, bool lean, int mode) {
                if (mode != DSIM_MODE_HELPER || (lean && !m->lean)) return;
                const size_t words = fwd ? m->lay.o.fwd_words : m->lay.o.total_words;
                int n = 0;
                ok = ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 2 * DSIM_NL, words * 4) == hipSuccess;
                if (n < per_cu) per_cu = n;
            });
            m->helper_max_envs = ok ? cus * per_cu : 0;
            if (const char* f = getenv("DSIM_HELPER")) m->helper_max_envs = atoi(f) ? (1 << 30) : 0;
        }
        if constexpr (dsim_has_mode<D, NW, true, DSIM_MODE_PAIR>()) {
            m->pair_min_envs = 0;
            if (const char* f = getenv("DSIM_PAIR")) m->pair_min_envs = atoi(f) ? 0 : (1 << 30);
        }
        return 0;
    });
}

extern "C" {

int dsim_model_destroy(dsim_model* m) {
    if (!m) return DSIM_OK;
    free_model(m);
    return DSIM_OK;
}

int dsim_model_status(dsim_model* m, int* first_env) {
    if (!m) return fail(DSIM_ERR_INVALID, "null model");
    if (first_env) *first_env = -1;
    if (m->h_status && m->h_status[0] != 0) {
        if (first_env) *first_env = m->h_status[1];
        return check_status(m);
    }
    return DSIM_OK;
}

int64_t dsim_ckpt_floats_mm(const dsim_model* m, int substeps, int mm_freq) {
    if (!m || substeps <= 0 || mm_freq <= 0) return 0;
    return (int64_t)dsim_ckpt_words(m->row_words(), m->lay.d.nq, m->lay.d.nd, substeps, mm_freq);
}

int64_t dsim_ckpt_floats(const dsim_model* m, int substeps) { return dsim_ckpt_floats_mm(m, substeps, 1); }

int dsim_model_set_ckpt_mode(dsim_model* m, int mode) {
    if (!m) return fail(DSIM_ERR_INVALID, "null model");
    if (mode != DSIM_CKPT_FULL && mode != DSIM_CKPT_LEAN) return fail(DSIM_ERR_INVALID, "unknown checkpoint mode");
    if (int rc = check_device(m)) return rc;   // the occupancy query below is per device
    m->lean = mode == DSIM_CKPT_LEAN;
    dsim_helper_capacity(m);
    return DSIM_OK;
}

int dsim_step_forward(const dsim_model* m, int n_envs, const float* q_in, const float* qd_in, const float* act,
                      const float* muscle_act, float dt, int substeps, int mm_freq, float* q_out, float* qd_out,
                      float* ckpt, void* hip_stream) {
    int rc = check_common(m, n_envs, dt, substeps, mm_freq);
    if (rc) return rc;
    if (!q_in || !qd_in || !act || !q_out || !qd_out) return fail(DSIM_ERR_INVALID, "null state pointer");
    if (m->lay.d.M > 0 && !muscle_act) return fail(DSIM_ERR_INVALID, "model has muscles but muscle_act is null");
    return launch_step<dsim_fwd_kernel_family>(m, n_envs, dt, substeps, mm_freq, hip_stream, q_in, qd_in, act, muscle_act, q_out,
                                               qd_out, ckpt);
}

static int step_backward(const dsim_model* m, int n_envs, const float* ckpt, const float* act, const float* muscle_act,
                         float dt, int substeps, int mm_freq, const float* gq_out, const float* gqd_out, float* gq_in,
                         float* gqd_in, float* gact, float* gmuscle_act, float* lit, void* hip_stream) {
    int rc = check_common(m, n_envs, dt, substeps, mm_freq);
    if (rc) return rc;
    if (!ckpt || !act || !gq_out || !gqd_out || !gq_in || !gqd_in)
        return fail(DSIM_ERR_INVALID, "null pointer (ckpt/act/grad)");
    if (m->lay.d.M > 0 && !muscle_act) return fail(DSIM_ERR_INVALID, "model has muscles but muscle_act is null");
    return launch_step<dsim_bwd_kernel_family>(m, n_envs, dt, substeps, mm_freq, hip_stream, ckpt, act, muscle_act, gq_out, gqd_out,
                                               gq_in, gqd_in, gact, gmuscle_act, lit);
}

int dsim_step_backward(const dsim_model* m, int n_envs, const float* ckpt, const float* act, const float* muscle_act,
                       float dt, int substeps, int mm_freq, const float* gq_out, const float* gqd_out, float* gq_in,
                       float* gqd_in, float* gact, float* gmuscle_act, void* hip_stream) {
    return step_backward(m, n_envs, ckpt, act, muscle_act, dt, substeps, mm_freq, gq_out, gqd_out, gq_in, gqd_in, gact, gmuscle_act,
                         nullptr, hip_stream);
}

// Largest grid of dsim_step_backward_multi / dsim_step_jacobian: n_envs * n_cot workgroups of up to 256 lanes, the launch's
// thread count below 2^32.
#define DSIM_MULTI_MAX_BLOCKS ((1ll << 24) - 1)

static int step_backward_multi(const dsim_model* m, int n_envs, float dt, int substeps, int mm_freq, const DsimMultiArgs& a,
                               void* hip_stream) {
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const unsigned blocks = (unsigned)((long long)n_envs * a.n_cot);
    return dispatch(m, [&](auto o, auto d, auto nw) {
        using O = decltype(o);
        using D = decltype(d);
        constexpr int NW = decltype(nw)::value;
        auto k = make_k(m, o, d, n_envs, dt, substeps, mm_freq);
        DsimMultiArgs args = a;
        args.ckpt_stride = k.ckpt_stride;
        const size_t bytes = (size_t)m->lay.o.total_words * 4;
        if (m->lean) hipLaunchKernelGGL((dsim_bwd_multi_kernel<O, D, NW, true>), dim3(blocks), dim3(DSIM_NL * NW), bytes, st, k, args);
        else hipLaunchKernelGGL((dsim_bwd_multi_kernel<O, D, NW, false>), dim3(blocks), dim3(DSIM_NL * NW), bytes, st, k, args);
        return launched("launch dsim_bwd_multi_kernel");
    });
}

static int check_multi(const dsim_model* m, int n_envs, int n_cot, const float* ckpt, const float* act, const float* muscle_act,
                       float dt, int substeps, int mm_freq) {
    int rc = check_common(m, n_envs, dt, substeps, mm_freq);
    if (rc) return rc;
    if (n_cot <= 0) return fail(DSIM_ERR_INVALID, "n_cot must be positive");
    if (!ckpt || !act) return fail(DSIM_ERR_INVALID, "null pointer (ckpt/act)");
    if (m->lay.d.M > 0 && !muscle_act) return fail(DSIM_ERR_INVALID, "model has muscles but muscle_act is null");
    if ((long long)n_envs * n_cot > DSIM_MULTI_MAX_BLOCKS)
        return fail(DSIM_ERR_LIMIT, "n_envs * n_cot = " + std::to_string((long long)n_envs * n_cot) + " workgroups exceed the grid limit of " +
                                        std::to_string(DSIM_MULTI_MAX_BLOCKS) + ": split the environments over several calls");
    return DSIM_OK;
}

int dsim_step_backward_multi(const dsim_model* m, int n_envs, int n_cot, int cot_shared, const float* ckpt, const float* act,
                             const float* muscle_act, float dt, int substeps, int mm_freq, const float* gq_out,
                             const float* gqd_out, float* gq_in, float* gqd_in, float* gact, float* gmuscle_act, void* hip_stream) {
    if (m && n_envs > 0 && n_cot > 0 && (!gq_out || !gqd_out || !gq_in || !gqd_in))
        return fail(DSIM_ERR_INVALID, "null pointer (grad)");
    int rc = check_multi(m, n_envs, n_cot, ckpt, act, muscle_act, dt, substeps, mm_freq);
    if (rc) return rc;
    const int nq = m->lay.d.nq, nd = m->lay.d.nd, M = m->lay.d.M;
    DsimMultiArgs a{};
    a.n_cot = n_cot; a.cot_shared = cot_shared != 0;
    a.ckpt = ckpt; a.act = act; a.mact = muscle_act;
    a.gq_out = gq_out; a.gqd_out = gqd_out; a.gq_out_stride = nq; a.gqd_out_stride = nd;
    a.gq_in = gq_in; a.gqd_in = gqd_in; a.gact = gact; a.gmact = gmuscle_act;
    a.gq_in_stride = nq; a.gqd_in_stride = nd; a.gact_stride = nd; a.gmact_stride = M;
    return step_backward_multi(m, n_envs, dt, substeps, mm_freq, a, hip_stream);
}

int dsim_step_jacobian(const dsim_model* m, int n_envs, const float* ckpt, const float* act, const float* muscle_act, float dt,
                       int substeps, int mm_freq, float* J_state, float* J_act, float* J_muscle, void* hip_stream) {
    if (m && n_envs > 0 && !J_state) return fail(DSIM_ERR_INVALID, "null pointer (J_state)");
    const int K = m ? m->lay.d.nq + m->lay.d.nd : 1;
    int rc = check_multi(m, n_envs, K, ckpt, act, muscle_act, dt, substeps, mm_freq);
    if (rc) return rc;
    const int nq = m->lay.d.nq, nd = m->lay.d.nd, M = m->lay.d.M;
    DsimMultiArgs a{};
    a.n_cot = K; a.cot_shared = 1;
    a.ckpt = ckpt; a.act = act; a.mact = muscle_act;
    a.gq_out = m->d_eye; a.gqd_out = m->d_eye + nq; a.gq_out_stride = K; a.gqd_out_stride = K;   // row k of the identity
    a.gq_in = J_state; a.gqd_in = J_state + nq; a.gact = J_act; a.gmact = J_muscle;              // [gq_in | gqd_in] = row k of J_state
    a.gq_in_stride = K; a.gqd_in_stride = K; a.gact_stride = nd; a.gmact_stride = M;
    return step_backward_multi(m, n_envs, dt, substeps, mm_freq, a, hip_stream);
}

// where a parameter array lies in the constant block: (word offset, floats), or false for an unknown field
static bool param_field(const dsim_model* m, int field, int& off, int& n) {
    const DsimOff& o = m->lay.o;
    const DsimDims& d = m->lay.d;
    switch (field) {
    case DSIM_PARAM_TARGET_KE: off = o.tke; n = d.L; return true;
    case DSIM_PARAM_TARGET_KD: off = o.tkd; n = d.L; return true;
    case DSIM_PARAM_LIMIT_KE: off = o.lke; n = d.L; return true;
    case DSIM_PARAM_LIMIT_KD: off = o.lkd; n = d.L; return true;
    case DSIM_PARAM_TARGET: off = o.target; n = d.nq; return true;
    case DSIM_PARAM_CONTACT_MATERIAL: off = o.cmat; n = 4 * d.C; return true;
    default: return false;
    }
}

// ONE launch: words [off, off + n) of rows 0 .. n_rows - 1 of the per-environment block <- values (src_stride floats apart; 0: the
// same array into every row).  The rows exist (n_rows <= env_rows) and [off, off + n) lies inside a row (param_field).
static int scatter_env_params(dsim_model* m, int off, int n, int n_rows, const float* values, long long src_stride, void* hip_stream) {
    const int bpr = (n + 63) / 64;
    hipLaunchKernelGGL(dsim_env_params_scatter_kernel, dim3((unsigned)((long long)n_rows * bpr)), dim3(64), 0,
                       static_cast<hipStream_t>(hip_stream), values, src_stride, m->d_env_cblob, m->env_words(), off, n, n_rows, bpr);
    return launched("launch dsim_env_params_scatter_kernel");
}

int dsim_model_set_params(dsim_model* m, int field, const float* dev_values, void* hip_stream) {
    if (!m) return fail(DSIM_ERR_INVALID, "null model");
    if (!dev_values) return fail(DSIM_ERR_INVALID, "null pointer (dev_values)");
    int off = 0, n = 0;
    if (!param_field(m, field, off, n)) return fail(DSIM_ERR_INVALID, "unknown parameter field " + std::to_string(field));
    if (int rc = check_device(m)) return rc;
    if (n == 0) return DSIM_OK;   // (contact materials of a model without contacts)
    // the six arrays are plain copies in the constant block (dsim_layout.hpp: put_f); nothing on the host is derived from them
    hipError_t e = hipMemcpyAsync(m->d_cblob + off, dev_values, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice,
                                  static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return hip_fail(e, "dsim_model_set_params");
    // per-environment mode: "for ALL environments" is every reserved row as well
    if (m->env_rows) return scatter_env_params(m, off, n, m->env_rows, dev_values, 0, hip_stream);
    return DSIM_OK;
}

int dsim_model_env_params(const dsim_model* m) { return m ? m->env_rows : 0; }

int dsim_model_reserve_env_params(dsim_model* m, int n_envs, void* hip_stream) {
    if (!m) return fail(DSIM_ERR_INVALID, "null model");
    if (n_envs < 0) return fail(DSIM_ERR_INVALID, "n_envs must not be negative");
    if (int rc = check_device(m)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // it allocates and frees: not something a captured graph can replay
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(st, &cap);
    if (e != hipSuccess || cap != hipStreamCaptureStatusNone) {
        if (e != hipSuccess) (void)hipGetLastError();
        return fail(DSIM_ERR_INVALID, "dsim_model_reserve_env_params allocates device memory and cannot run while a stream capture is "
                                      "active: reserve before the capture begins");
    }
    if (n_envs != m->env_rows && m->d_env_cblob) {   // (hipFree waits for the launches that still read the rows)
        uint32_t* old = m->d_env_cblob;
        m->d_env_cblob = nullptr;
        m->env_rows = 0;
        e = hipFree(old);
        if (e != hipSuccess) return hip_fail(e, "dsim_model_reserve_env_params (hipFree)");
    }
    if (n_envs == 0) return DSIM_OK;
    const int W = m->env_words();
    if (!m->d_env_cblob) {
        e = hipMalloc(&m->d_env_cblob, sizeof(uint32_t) * (size_t)W * (size_t)n_envs);
        if (e != hipSuccess) {
            m->d_env_cblob = nullptr;
            return hip_fail(e, "dsim_model_reserve_env_params (hipMalloc)");
        }
    }
    hipLaunchKernelGGL(dsim_env_params_fill_kernel, dim3((unsigned)n_envs), dim3(64), 0, st, m->d_cblob, m->d_env_cblob, W, n_envs);
    if (int rc = launched("launch dsim_env_params_fill_kernel")) {
        if (!m->env_rows) {
            (void)hipFree(m->d_env_cblob);
            m->d_env_cblob = nullptr;
        }
        return rc;
    }
    m->env_rows = n_envs;
    return DSIM_OK;
}

int dsim_model_set_env_params(dsim_model* m, int field, int n_envs, const float* dev_values, void* hip_stream) {
    if (!m) return fail(DSIM_ERR_INVALID, "null model");
    if (!dev_values) return fail(DSIM_ERR_INVALID, "null pointer (dev_values)");
    int off = 0, n = 0;
    if (!param_field(m, field, off, n)) return fail(DSIM_ERR_INVALID, "unknown parameter field " + std::to_string(field));
    if (!m->env_rows)
        return fail(DSIM_ERR_INVALID, "the model shares one parameter block between all environments: dsim_model_reserve_env_params first");
    if (n_envs < 1 || n_envs > m->env_rows)
        return fail(DSIM_ERR_INVALID, "n_envs = " + std::to_string(n_envs) + " is outside 1 .. " + std::to_string(m->env_rows) +
                                          ", the environments the model holds per-environment parameters for");
    if (int rc = check_device(m)) return rc;
    if (n == 0) return DSIM_OK;   // (contact materials of a model without contacts)
    return scatter_env_params(m, off, n, n_envs, dev_values, n, hip_stream);
}

int dsim_step_backward_params(const dsim_model* m, int n_envs, const float* ckpt, const float* act, const float* muscle_act,
                              float dt, int substeps, int mm_freq, const float* gq_out, const float* gqd_out, float* gq_in,
                              float* gqd_in, float* gact, float* gmuscle_act, float* g_dof, float* g_contact, void* hip_stream) {
    int rc = check_common(m, n_envs, dt, substeps, mm_freq);
    if (rc) return rc;
    if (!ckpt || !act || !gq_out || !gqd_out || !gq_in || !gqd_in) return fail(DSIM_ERR_INVALID, "null pointer (ckpt/act/grad)");
    if (m->lay.d.M > 0 && !muscle_act) return fail(DSIM_ERR_INVALID, "model has muscles but muscle_act is null");
    if (!g_dof && !g_contact) return fail(DSIM_ERR_INVALID, "g_dof and g_contact are both null (dsim_step_backward is that call)");
    const size_t bytes = ((size_t)m->lay.o.total_words + (size_t)(5 * m->lay.d.nd + 4 * m->lay.d.C)) * 4;   // + dsim_par_words(nd, C)
    if (bytes > 160 * 1024) return fail(DSIM_ERR_LIMIT, "model needs more than 160 KiB of LDS per environment with the parameter accumulators");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return dispatch(m, [&](auto o, auto d, auto nw) {
        using O = decltype(o);
        using D = decltype(d);
        constexpr int NW = decltype(nw)::value;
        auto k = make_k(m, o, d, n_envs, dt, substeps, mm_freq);
        const DsimParArgs a{ckpt, act, muscle_act, gq_out, gqd_out, gq_in, gqd_in, gact, gmuscle_act, g_dof, g_contact};
        if (m->lean) hipLaunchKernelGGL((dsim_bwd_param_kernel<O, D, NW, true>), dim3(n_envs), dim3(DSIM_NL * NW), bytes, st, k, a);
        else hipLaunchKernelGGL((dsim_bwd_param_kernel<O, D, NW, false>), dim3(n_envs), dim3(DSIM_NL * NW), bytes, st, k, a);
        return launched("launch dsim_bwd_param_kernel");
    });
}

int64_t dsim_literal_scratch_floats(const dsim_model* m) {
    if (!m) return 0;
    const int64_t nq = m->lay.d.nq, nd = m->lay.d.nd;
    return nq + nd + nd * nd;
}

int dsim_step_backward_literal(const dsim_model* m, int n_envs, const float* ckpt, const float* act, const float* muscle_act,
                               float dt, int substeps, int mm_freq, const float* gq_out, const float* gqd_out, float* gq_in,
                               float* gqd_in, float* gact, float* gmuscle_act, float* scratch, void* hip_stream) {
    if (!m) return fail(DSIM_ERR_INVALID, "null model");
    if (!scratch) return fail(DSIM_ERR_INVALID, "null scratch (n_envs x dsim_literal_scratch_floats(m) floats)");
    if (m->lay.d.L > DSIM_LIT_LMAX || m->lay.d.nd > DSIM_LIT_NDMAX)
        return fail(DSIM_ERR_LIMIT, "dsim_step_backward_literal handles models of up to " + std::to_string(DSIM_LIT_LMAX) + " links and " +
                                        std::to_string(DSIM_LIT_NDMAX) + " dofs");
    int rc = step_backward(m, n_envs, ckpt, act, muscle_act, dt, substeps, mm_freq, gq_out, gqd_out, gq_in, gqd_in, gact, gmuscle_act,
                           scratch, hip_stream);
    if (rc) return rc;
    if ((m->lay.d.tmask & (DSIM_TM(DSIM_JOINT_BALL) | DSIM_TM(DSIM_JOINT_FREE))) == 0) return DSIM_OK;   // no quaternion coordinates
    auto k = make_k(m, m->lay.o, m->lay.d, n_envs, dt, substeps, mm_freq);
    const long long threads = (long long)n_envs * m->lay.d.L;
    hipLaunchKernelGGL(dsim_literal_radial_kernel, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(hip_stream), k,
                       m->row_words(), ckpt, act, muscle_act, scratch, gq_in);
    return launched("launch dsim_literal_radial_kernel");
}

int dsim_env_step_forward(const dsim_model* m, const dsim_env_spec* env, int n_envs, const float* q_in,
                          const float* qd_in, const float* actions, float dt, int substeps, int mm_freq, float* q_out,
                          float* qd_out, float* obs, float* rew, float* ckpt, const dsim_episode* episode,
                          void* hip_stream) {
    int rc = check_common(m, n_envs, dt, substeps, mm_freq);
    if (rc) return rc;
    DsimEnvSpec sp;
    rc = make_spec(m, env, sp);
    if (rc) return rc;
    if (!q_in || !qd_in || !actions || !q_out || !qd_out || !obs || !rew) return fail(DSIM_ERR_INVALID, "null pointer");
    DsimEpisode ep{};
    if (episode) {
        if (!episode->progress || !episode->done || !episode->reset_q || !episode->reset_qd || !episode->reset_count)
            return fail(DSIM_ERR_INVALID, "episode: null pointer (progress/done/reset_q/reset_qd/reset_count)");
        if (episode->reset_pool <= 0) return fail(DSIM_ERR_INVALID, "episode: reset_pool must be positive");
        if (episode->episode_length <= 0) return fail(DSIM_ERR_INVALID, "episode: episode_length must be positive");
        ep = dsim_episode_copy(*episode);
    }
    return launch_step<dsim_env_fwd_kernel_family>(m, n_envs, dt, substeps, mm_freq, hip_stream, sp, ep, q_in, qd_in, actions, q_out,
                                                   qd_out, obs, rew, ckpt);
}

int dsim_env_step_backward(const dsim_model* m, const dsim_env_spec* env, int n_envs, const float* ckpt,
                           const float* actions, float dt, int substeps, int mm_freq, const float* gq_out,
                           const float* gqd_out, const float* gobs, const float* grew, const float* gobs_before_reset,
                           float* gq_in, float* gqd_in, float* gactions, void* hip_stream) {
    int rc = check_common(m, n_envs, dt, substeps, mm_freq);
    if (rc) return rc;
    DsimEnvSpec sp;
    rc = make_spec(m, env, sp);
    if (rc) return rc;
    if (!ckpt || !actions || !gq_in || !gqd_in || !gactions) return fail(DSIM_ERR_INVALID, "null pointer");
    return launch_step<dsim_env_bwd_kernel_family>(m, n_envs, dt, substeps, mm_freq, hip_stream, sp, ckpt, actions, gq_out, gqd_out,
                                                   gobs, grew, gobs_before_reset, gq_in, gqd_in, gactions);
}

int dsim_env_step_backward_params(const dsim_model* m, const dsim_env_spec* env, int n_envs, const float* ckpt,
                                  const float* actions, float dt, int substeps, int mm_freq, const float* gq_out,
                                  const float* gqd_out, const float* gobs, const float* grew, const float* gobs_before_reset,
                                  float* gq_in, float* gqd_in, float* gactions, float* g_dof, float* g_contact, void* hip_stream) {
    int rc = check_common(m, n_envs, dt, substeps, mm_freq);
    if (rc) return rc;
    DsimEnvSpec sp;
    rc = make_spec(m, env, sp);
    if (rc) return rc;
    if (!ckpt || !actions || !gq_in || !gqd_in || !gactions) return fail(DSIM_ERR_INVALID, "null pointer");
    const size_t bytes = ((size_t)m->lay.o.total_words + (size_t)(5 * m->lay.d.nd + 4 * m->lay.d.C)) * 4;   // + dsim_par_words(nd, C)
    if (bytes > 160 * 1024) return fail(DSIM_ERR_LIMIT, "model needs more than 160 KiB of LDS per environment with the parameter accumulators");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return dispatch(m, [&](auto o, auto d, auto nw) {
        using O = decltype(o);
        using D = decltype(d);
        constexpr int NW = decltype(nw)::value;
        auto k = make_k(m, o, d, n_envs, dt, substeps, mm_freq);
        const DsimEnvParArgs a{ckpt, actions, gq_out, gqd_out, gobs, grew, gobs_before_reset, gq_in, gqd_in, gactions, g_dof, g_contact};
        if (m->lean) hipLaunchKernelGGL((dsim_env_bwd_param_kernel<O, D, NW, true>), dim3(n_envs), dim3(DSIM_NL * NW), bytes, st, k, sp, a);
        else hipLaunchKernelGGL((dsim_env_bwd_param_kernel<O, D, NW, false>), dim3(n_envs), dim3(DSIM_NL * NW), bytes, st, k, sp, a);
        return launched("launch dsim_env_bwd_param_kernel");
    });
}

int dsim_env_observe(const dsim_model* m, const dsim_env_spec* env, int n_envs, const float* q, const float* qd,
                     const float* stored_actions, float* obs, float* rew, void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    DsimEnvSpec sp;
    rc = make_spec(m, env, sp);
    if (rc) return rc;
    if (!q || !qd || !stored_actions || !obs || !rew) return fail(DSIM_ERR_INVALID, "null pointer");
    return launch_readout<dsim_env_obs_kernel_family>(m, n_envs, hip_stream, sp, q, qd, stored_actions, obs, rew);
}

int dsim_body_transforms(const dsim_model* m, int n_envs, const float* q, float* X_sc, float* X_sm, void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    if (!q || !X_sc) return fail(DSIM_ERR_INVALID, "null pointer");
    return launch_readout<dsim_body_xf_family>(m, n_envs, hip_stream, q, (const float*)nullptr, X_sc, X_sm, (float*)nullptr);
}

int dsim_body_kinematics(const dsim_model* m, int n_envs, const float* q, const float* qd, float* X_sc, float* X_sm, float* v_s,
                         void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    if (!q || !X_sc) return fail(DSIM_ERR_INVALID, "null pointer");
    if ((qd == nullptr) != (v_s == nullptr)) return fail(DSIM_ERR_INVALID, "v_s is returned if and only if qd is given");
    return launch_readout<dsim_body_kin_kernel_family>(m, n_envs, hip_stream, q, qd, X_sc, X_sm, v_s);
}

int dsim_body_kinematics_backward(const dsim_model* m, int n_envs, const float* q, const float* qd, const float* gX_sc,
                                  const float* gX_sm, const float* gv_s, float* gq, float* gqd, void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    if (!q || !gq) return fail(DSIM_ERR_INVALID, "null pointer");
    if ((qd == nullptr) != (gqd == nullptr)) return fail(DSIM_ERR_INVALID, "gqd is returned if and only if qd is given");
    if (!qd && gv_s) return fail(DSIM_ERR_INVALID, "gv_s without qd: there is no v_s output to have a cotangent");
    return launch_readout<dsim_body_kin_bwd_kernel_family>(m, n_envs, hip_stream, q, qd, gX_sc, gX_sm, gv_s, gq, gqd);
}

int dsim_joint_dynamics(const dsim_model* m, int n_envs, const float* q, const float* qd, const float* act, const float* muscle_act,
                        float* tau, float* qdd, float* f_s, void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    if (!q || !qd) return fail(DSIM_ERR_INVALID, "null pointer");
    if (!tau && !qdd && !f_s) return fail(DSIM_ERR_INVALID, "no output: tau, qdd and f_s are all null");
    return launch_readout<dsim_joint_dyn_kernel_family>(m, n_envs, hip_stream, q, qd, act, muscle_act, tau, qdd, f_s);
}

int dsim_joint_dynamics_backward(const dsim_model* m, int n_envs, const float* q, const float* qd, const float* act,
                                 const float* muscle_act, const float* gtau, const float* gqdd, const float* gf_s, float* gq,
                                 float* gqd, float* gact, float* gmuscle_act, void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    if (!q || !qd || !gq || !gqd) return fail(DSIM_ERR_INVALID, "null pointer");
    return launch_readout<dsim_joint_dyn_bwd_kernel_family>(m, n_envs, hip_stream, q, qd, act, muscle_act, gtau, gqdd, gf_s, gq, gqd,
                                                            gact, gmuscle_act);
}

int dsim_ground_contacts(const dsim_model* m, int n_envs, const float* q, const float* qd, float* point, float* vel, float* force,
                         float* link_wrench, void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    if (!q || !qd) return fail(DSIM_ERR_INVALID, "null pointer");
    if (!point && !vel && !force && !link_wrench)
        return fail(DSIM_ERR_INVALID, "no output: point, vel, force and link_wrench are all null");
    return launch_readout<dsim_ground_con_kernel_family>(m, n_envs, hip_stream, q, qd, point, vel, force, link_wrench);
}

int dsim_ground_contacts_backward(const dsim_model* m, int n_envs, const float* q, const float* qd, const float* gpoint,
                                  const float* gvel, const float* gforce, const float* glink_wrench, float* gq, float* gqd,
                                  void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    if (!q || !qd || !gq || !gqd) return fail(DSIM_ERR_INVALID, "null pointer");
    return launch_readout<dsim_ground_con_bwd_kernel_family>(m, n_envs, hip_stream, q, qd, gpoint, gvel, gforce, glink_wrench, gq,
                                                             gqd);
}

int dsim_mass_matrix(const dsim_model* m, int n_envs, const float* q, float* H, float* Hinv, float* S, void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    if (!q) return fail(DSIM_ERR_INVALID, "null pointer");
    if (!H && !Hinv && !S) return fail(DSIM_ERR_INVALID, "no output: H, Hinv and S are all null");
    return launch_readout<dsim_mass_kernel_family>(m, n_envs, hip_stream, q, H, Hinv, S);
}

int dsim_mass_matrix_backward(const dsim_model* m, int n_envs, const float* q, const float* gH, const float* gHinv, const float* gS,
                              float* gq, void* hip_stream) {
    int rc = check_common(m, n_envs, 1.0f, 1, 1);
    if (rc) return rc;
    if (!q || !gq) return fail(DSIM_ERR_INVALID, "null pointer");
    return launch_readout<dsim_mass_bwd_kernel_family>(m, n_envs, hip_stream, q, gH, gHinv, gS, gq);
}

/* 0 = generic kernels, >0 = index of the specialised variant in use (diagnostics / tests) */
int dsim_model_variant(const dsim_model* m) { return m ? m->variant : -1; }
int dsim_model_waves(const dsim_model* m) { return m ? m->waves : -1; }
int dsim_model_device(const dsim_model* m) { return m ? m->device : -1; }

#ifdef DSIM_STAMPS
int dsim_debug_stamps(long long* out, int n) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dsim_stamps), sizeof(long long) * (size_t)(n < 2 * 16384 ? n : 2 * 16384));
    if (e == hipSuccess) {   // (cleared for the next launch: a shorter launch would otherwise end in the previous one's stamps)
        void* sym = nullptr;
        e = hipGetSymbolAddress(&sym, HIP_SYMBOL(g_dsim_stamps));
        if (e == hipSuccess) e = hipMemset(sym, 0, sizeof(long long) * 2 * 16384);
    }
    return e == hipSuccess ? DSIM_OK : hip_fail(e, "dsim_debug_stamps");
}
#endif

}  // extern "C"
