// fv3net_amd — vertical remap `mappm` on gfx950.
//
// Replaces the f2py-wrapped Fortran mappm (external/mappm/mappm/mappm.f90:10-126)
// as called by vcm.cubedsphere.regrid_vertical (external/vcm/vcm/cubedsphere/regridz.py:273).
//
// The column-fastest [level][column] layout (Fortran's pe1(i,k)) makes every per-level
// load a coalesced 256 B wave access.  The per-column algorithm is the one-pass streaming
// formulation in mappm_core.h / mappm_multi.h.  kord <= 7 (ppm_profile) has four kernels,
// all with the one-lane kernel's bits; ppm_kernel_choice (mappm_choice.h) picks one from
// the fields per launch, the column count and the device's CUs:
//   * mappm_ppm_levels_kernel: one block per column, a lane per level, for grids too small
//     to fill the chip with columns (one field per launch);
//   * mappm_ppm_pair_split_kernel<NF, K1, 3> and <NF, K1, 2>: one or two fields with three
//     or two lanes per column, each streaming a share of the outputs, while all their waves
//     are resident (the default from 10,240 columns for pairs, 20,480 for one field);
//   * mappm_ppm_kernel (one field) and mappm_ppm_pair_kernel (two): one lane per column,
//     entirely in registers (no LDS, no scratch), on the large grids.
// kord > 7 solves cs_profile's tridiagonal edge system into a [2][km+3][column] scratch in
// global memory (coalesced; LDS kept behind FV3_MAPPM_LDS), then streams.
// Roofline: HBM-bound at (km+1 + km + kn+1 + kn) * 4 B per column, with ~150
// VALU ops per input level (including ~7 IEEE divides) close behind.
#define FV3_HD __host__ __device__
#include "common.h"
#include "mappm_choice.h"
#include "mappm_core.h"
#include "mappm_multi.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace fv3 {

// launch arguments, shared by the exact and the fast-arithmetic translation units
// (mappm.hip, mappm_fast.hip: the same kernels under mappm_core.h's two policies)
struct MappmArgs {
    const float* pe1;
    const float* q1;
    const float* pe2;
    float* q2;
    fv3_layout l_pe1, l_q1, l_pe2, l_q2;
    int64_t ncol;
    int km, kn, iv, kord;
    float* scratch;  // kord > 7: [2][km+3][grid * block] (NULL: the LDS path)
};

struct MappmPairArgs {
    const float* pe1;
    const float* pe2;
    fv3_layout l_pe1, l_pe2;
    const float* q1[2];
    float* q2[2];
    fv3_layout l_q1[2], l_q2[2];
    int64_t ncol;
    int km, kn, iv, kord;
};

// CUs of the current device, queried once (thread-safe static initialisation)
inline int device_cus()
{
    static const int n_cu = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        return n;
    }();
    return n_cu;
}

// the kord <= 7 kernel of a launch of `fields` fields on this device (mappm_choice.h); the
// knobs of the choice are read here and nowhere else
inline PpmKernel ppm_kernel(int fields, int64_t ncol, int km, int kn)
{
    const PpmKnobs knobs{variant_env("FV3_MAPPM_PATH"), variant_env("FV3_MAPPM_SPLIT"),
                         variant_env("FV3_MAPPM_SPLIT1")};
    return ppm_kernel_choice(fields, ncol, km, kn, device_cus(), knobs);
}

namespace FV3_ARITH_NS {
int launch_mappm(MappmArgs a, hipStream_t stream);
int launch_mappm_pairs(MappmPairArgs a, int lanes, hipStream_t stream);
}  // namespace FV3_ARITH_NS
#ifndef FV3_FAST_ARITH
namespace fast {  // mappm_fast.hip
int launch_mappm(MappmArgs a, hipStream_t stream);
int launch_mappm_pairs(MappmPairArgs a, int lanes, hipStream_t stream);
}  // namespace fast
#endif

namespace FV3_ARITH_NS {  // kernels named fv3::exact::... / fv3::fast::... in traces
namespace {

// The remap consumer emits q2(k) for k = 1, 2, ... and asks for next_edge(k) for
// k = 2, 3, ... strictly in order, so both walk running pointers: no per-lane 64-bit
// index multiply per output level.
#ifndef FV3_MAPPM_EDGE_AHEAD
#define FV3_MAPPM_EDGE_AHEAD 1  // next_edge's load one call ahead (0: tools A/B builds)
#endif

struct EdgeCursor {
    const float* pe2_;
    int64_t ld_pe2;
    int kn;
    const float* pe2_next;  // the edge after nb
    float nb;               // pe2(k + 1) for the next next_edge(k), loaded one call ahead
    __device__ __forceinline__ float pe2(int k) const { return pe2_[(int64_t)(k - 1) * ld_pe2]; }
    // the cursor where the single pass has it when it begins output k_first (1: a whole column)
    __device__ __forceinline__ void seek(int k_first)
    {
        pe2_next = pe2_ + (int64_t)(k_first + 1) * ld_pe2;
        nb = (k_first + 2 <= kn + 1) ? *pe2_next : 0.0f;
    }
    __device__ __forceinline__ float next_edge(int k)
    {
        if (k + 1 > kn + 1) return 0.0f;
#if FV3_MAPPM_EDGE_AHEAD
        const float r = nb;
        pe2_next += ld_pe2;
        nb = (k + 2 <= kn + 1) ? *pe2_next : 0.0f;
#else  // A/B variant builds: loaded at the call
        const float r = *pe2_next;
        pe2_next += ld_pe2;
#endif
        return r;
    }
};

struct DevCol {
    const float* pe1_;
    const float* q1_;
    float* q2_;
    int64_t ld_pe1, ld_q1, ld_q2;
    EdgeCursor edge;
    __device__ __forceinline__ float pe2(int k) const { return edge.pe2(k); }
    __device__ __forceinline__ float next_edge(int k) { return edge.next_edge(k); }
    __device__ __forceinline__ float q1(int k) const { return q1_[(int64_t)(k - 1) * ld_q1]; }
    __device__ __forceinline__ float pe1(int k) const { return pe1_[(int64_t)(k - 1) * ld_pe1]; }
    __device__ __forceinline__ void emit(int, float v)
    {
        *q2_ = v;
        q2_ += ld_q2;
    }
};

// DevCol with buffer loads: q1(k) / pe1(k) at a uniform level k are one
// `buffer_load_dword` of (resource over the array) + (the lane's byte offset, VGPR) +
// (the level's byte offset, SGPR soffset), so every load in flight holds one data VGPR
// and no 64-bit address (DevCol's each hold an address pair, which the compiler does not
// fold into a uniform-base form by itself).  The host checks every array spans < 4 GiB.
// emit / next_edge walk per-lane pointers as in DevCol.
typedef __amdgpu_buffer_rsrc_t MRsrc;
__device__ __forceinline__ MRsrc mrsrc(const void* p)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0xffffffffu, 0x00020000);
}
__device__ __forceinline__ float bload(MRsrc r, uint32_t voff, uint32_t soff)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}

struct DevColBuf {
    MRsrc r_pe1, r_q1;
    uint32_t o_pe1, o_q1;     // lane byte offsets
    uint32_t lb_pe1, lb_q1;   // level strides in bytes
    float* q2_;
    int64_t ld_q2;
    EdgeCursor edge;
    __device__ __forceinline__ float pe2(int k) const { return edge.pe2(k); }
    __device__ __forceinline__ float next_edge(int k) { return edge.next_edge(k); }
    __device__ __forceinline__ float q1(int k) const { return bload(r_q1, o_q1, (uint32_t)(k - 1) * lb_q1); }
    __device__ __forceinline__ float pe1(int k) const { return bload(r_pe1, o_pe1, (uint32_t)(k - 1) * lb_pe1); }
    __device__ __forceinline__ void emit(int, float v)
    {
        *q2_ = v;
        q2_ += ld_q2;
    }
};

// GlobalScr through buffer loads / stores (the host checks the scratch is < 4 GiB);
// e(k) / g(k) are proxies: read as a float, assigned by a store
struct GlobalScrBuf {
    MRsrc r;
    uint32_t o;   // lane byte offset
    uint32_t sb;  // level stride in bytes
    uint32_t pb;  // plane stride in bytes
    struct Ref {
        MRsrc r;
        uint32_t o, so;
        __device__ __forceinline__ operator float() const { return bload(r, o, so); }
        __device__ __forceinline__ Ref& operator=(float v)
        {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)o, (int)so, 0);
            return *this;
        }
    };
    __device__ __forceinline__ Ref e(int k) const { return Ref{r, o, (uint32_t)k * sb}; }
    __device__ __forceinline__ Ref g(int k) const { return Ref{r, o, pb + (uint32_t)k * sb}; }
};

struct LdsScr {
    float* base;  // [2][km+3][blockDim]
    int stride;   // blockDim.x
    int plane;    // (km+3) * blockDim.x
    __device__ __forceinline__ float& e(int k) { return base[k * stride]; }
    __device__ __forceinline__ float& g(int k) { return base[plane + k * stride]; }
};

// The same [2][km+3][column] scratch in global memory (stream-ordered allocation):
// coalesced like the column arrays, and unlike LDS (42 KB per 64 columns at km = 79,
// i.e. 3 waves per CU) it leaves occupancy to the VGPR budget.
struct GlobalScr {
    float* base;     // scratch + column
    int64_t stride;  // padded column count
    int64_t plane;   // (km+3) * stride
    __device__ __forceinline__ float& e(int k) { return base[k * stride]; }
    __device__ __forceinline__ float& g(int k) { return base[plane + k * stride]; }
};

__device__ __forceinline__ DevCol make_col(const MappmArgs& a, int64_t c)
{
    DevCol d;
    d.pe1_ = a.pe1 + col_offset(a.l_pe1, c);
    d.q1_ = a.q1 + col_offset(a.l_q1, c);
    d.edge.pe2_ = a.pe2 + col_offset(a.l_pe2, c);
    d.q2_ = a.q2 + col_offset(a.l_q2, c);
    d.ld_pe1 = a.l_pe1.ld;
    d.ld_q1 = a.l_q1.ld;
    d.edge.ld_pe2 = a.l_pe2.ld;
    d.ld_q2 = a.l_q2.ld;
    d.edge.kn = a.kn;
    d.edge.seek(1);
    return d;
}

// DevColBuf of column c: q1 / pe1 through buffer loads at 32-bit offsets (the host checks
// fits_c32), pe2 / q2 through per-lane pointers as in DevCol
__device__ __forceinline__ DevColBuf make_col_buf(const MappmArgs& a, int64_t c)
{
    DevColBuf d;
    d.r_pe1 = mrsrc(a.pe1);
    d.r_q1 = mrsrc(a.q1);
    d.o_pe1 = (uint32_t)(col_offset(a.l_pe1, c) * 4);
    d.o_q1 = (uint32_t)(col_offset(a.l_q1, c) * 4);
    d.lb_pe1 = (uint32_t)(a.l_pe1.ld * 4);
    d.lb_q1 = (uint32_t)(a.l_q1.ld * 4);
    d.edge.pe2_ = a.pe2 + col_offset(a.l_pe2, c);
    d.q2_ = a.q2 + col_offset(a.l_q2, c);
    d.edge.ld_pe2 = a.l_pe2.ld;
    d.ld_q2 = a.l_q2.ld;
    d.edge.kn = a.kn;
    d.edge.seek(1);
    return d;
}

// buffer operations at 32-bit byte offsets reach every element of an array in layout l
// over ncol columns and nlev levels: its last column's offset plus nlev levels < 4 GiB
inline bool fits_c32(const fv3_layout& l, int64_t ncol, int nlev)
{
    if (l.ld < 0 || l.blk_stride < 0) return false;
    const int64_t c = ncol - 1;
    const int64_t off = (l.ncol_blk <= 0 || c < l.ncol_blk) ? c : (c / l.ncol_blk) * l.blk_stride + c % l.ncol_blk;
    return 4 * (off + (int64_t)nlev * l.ld) < (1ll << 32) - 4;
}

// the single-field column's window in register rings (mappm_core.h, RING): on the fast
// arithmetic only, where it measured faster (0.384 -> 0.367 ms at C384 kord 1)
#ifdef FV3_FAST_ARITH
constexpr bool kRingWindow = true;
#else
constexpr bool kRingWindow = false;
#endif

// K1: kord 1 and iv 1 (the default of regrid_vertical and of the pressure-level coarsen)
// as compile-time constants, so every branch of mappm.f90 on kord / iv folds away
// BUF: q1 / pe1 through buffer loads at SGPR level offsets (DevColBuf), when every array
// fits 32-bit offsets; else 64-bit addresses.  C384 kord 1: fast 0.370 -> 0.368 ms, exact
// 0.501 -> 0.497 (profiles/r06zt_mappm_buf_ab.log)
#ifndef FV3_MAPPM_PPM_WPE
#define FV3_MAPPM_PPM_WPE 0  // register target in waves per SIMD (0: the compiler's, 66 VGPRs, 7 waves;
                             // 8 spills 5 and measured 0.365 -> 0.398 ms, profiles/r06zu_mappm_wpe_ab.log)
#endif
#if FV3_MAPPM_PPM_WPE
#define FV3_PPM_WPE_ATTR __attribute__((amdgpu_waves_per_eu(FV3_MAPPM_PPM_WPE, FV3_MAPPM_PPM_WPE)))
#else
#define FV3_PPM_WPE_ATTR
#endif
template <bool K1, bool BUF>
__global__ __launch_bounds__(256) FV3_PPM_WPE_ATTR void mappm_ppm_kernel(MappmArgs a)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    if constexpr (BUF) {
        DevColBuf col = make_col_buf(a, c);
        mappm_ppm_column<DevColBuf, true, true, kRingWindow>(col, a.km, a.kn, K1 ? 1 : a.iv, K1 ? 1 : a.kord);
    } else {
        DevCol col = make_col(a, c);
        mappm_ppm_column<DevCol, true, true, kRingWindow>(col, a.km, a.kn, K1 ? 1 : a.iv, K1 ? 1 : a.kord);
    }
}

// the K1 / general pick of a launch: kernel_of(std::true_type / std::false_type) names the
// kernel of either build
template <class F>
const void* pick_k1(int iv, int kord, F kernel_of)
{
    return (iv == 1 && kord == 1) ? kernel_of(std::true_type{}) : kernel_of(std::false_type{});
}

// No-op edge source for remap_one (the level-parallel kernel finishes one output
// layer per lane, so the next edge is never read).
struct NoEdge {
    __device__ __forceinline__ float next_edge(int) const { return 0.0f; }
};

// kord <= 7 with one BLOCK per column and one lane per level: the latency-bound
// case (config #1: 864 columns = 14 waves of the one-lane-per-column kernel, each
// walking 79 levels serially).  ppm_profile is a local stencil, so each phase below
// evaluates one of mappm_ppm_column's per-level expressions for every level at once,
// with the same helpers and operands, into LDS; the remap then gives each output
// layer its own lane, which replays remap_one over the input layers it overlaps
// (mappm.f90:58-124 for one k).  The streaming code starts output k's layer search
// where output k-1 ended; with non-decreasing pe1 and pe2 that is the first L with
// pe2(k) <= pe1(L+1), found here by bisection.  A column whose edges are not
// non-decreasing (or hold NaNs) runs the serial streaming code on lane 0 instead, so
// every input gives the serial kernel's (bit-exact) result.
//
// LDS: 9 (km+2) + (kn+2) floats, 1-based levels.
__global__ __launch_bounds__(128) void mappm_ppm_levels_kernel(MappmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int km = a.km, kn = a.kn, n = km + 2;
    const int tid = threadIdx.x, nt = blockDim.x;
    float* const q = lds;
    float* const pe = lds + n;
    float* const dp = lds + 2 * n;
    float* const dc = lds + 3 * n;
    float* const al = lds + 4 * n;  // AL(k); al[km+1] holds ar_km
    float* const h2 = lds + 5 * n;
    float* const pal = lds + 6 * n;  // final layer coefficients
    float* const par = lds + 7 * n;
    float* const pa6 = lds + 8 * n;
    float* const pe2 = lds + 9 * n;
    const int64_t c = blockIdx.x;
    DevCol col = make_col(a, c);

    for (int k = tid + 1; k <= km + 1; k += nt) {
        pe[k] = col.pe1(k);
        if (k <= km) q[k] = col.q1(k);
    }
    for (int k = tid + 1; k <= kn + 1; k += nt) pe2[k] = col.pe2(k);
    __syncthreads();
    int sorted = 1;
    for (int k = tid + 1; k <= km; k += nt) {
        dp[k] = pe[k + 1] - pe[k];
        sorted &= pe[k] <= pe[k + 1];
    }
    for (int k = tid + 1; k <= kn; k += nt) sorted &= pe2[k] <= pe2[k + 1];
    if (!__syncthreads_and(sorted)) {
        if (tid == 0) mappm_ppm_column(col, km, kn, a.iv, a.kord);
        return;
    }
    const int iv = a.iv, kord = a.kord;
    const bool huynh = kord >= 7;
    // dc(k), k = 2..km-1 (mappm.f90:658-668)
    for (int k = tid + 2; k <= km - 1; k += nt) dc[k] = ppm_dc(q[k - 1], q[k], q[k + 1], dp[k - 1], dp[k], dp[k + 1]);
    __syncthreads();
    // ALraw(m), m = 3..km-1 (mappm.f90:674-683)
    for (int m = tid + 3; m <= km - 1; m += nt)
        al[m] = ppm_al(dp[m - 2], dp[m - 1], dp[m], dp[m + 1], q[m - 1], q[m], dc[m - 1], dc[m]);
    __syncthreads();
    if (tid == 0) {  // top: area-preserving cubic (mappm.f90:689-725), as in mappm_ppm_column
        float al1, al2, dc1;
        ppm_top_cubic(q[1], q[2], dp[1], dp[2], al[3], iv, al1, al2, dc1);
        dc[1] = dc1;
        al[1] = al1;
        al[2] = al2;
    }
    if (tid == (1 % nt)) {  // bottom: area-preserving cubic (mappm.f90:729-761)
        float alm, ar, dcm;
        ppm_bottom_cubic(q[km], q[km - 1], dp[km], dp[km - 1], al[km - 1], iv, alm, ar, dcm);
        dc[km] = dcm;
        al[km] = alm;
        al[km + 1] = ar;
    }
    __syncthreads();
    if (huynh) {  // h2(k), k = 2..km-1 (mappm.f90:784-795)
        for (int k = tid + 2; k <= km - 1; k += nt) h2[k] = ppm_h2(dc[k - 1], dc[k + 1], dp[k - 1], dp[k], dp[k + 1]);
        __syncthreads();
    }
    int lmt = kord - 3;
    lmt = lmt > 0 ? lmt : 0;
    if (iv == 0) lmt = lmt < 2 ? lmt : 2;
    // final coefficients of every layer (the top of mappm_ppm_column's L loop)
    for (int L = tid + 1; L <= km; L += nt) {
        Ppm p{q[L], al[L], al[L + 1], 0.0f};  // al[km+1] = ar_km
        const float dcL = dc[L];
        if (L <= 2 || L >= km - 1) {
            p.a6 = a6_of(p);
            ppm_limit(dcL, p, 0);
        } else if (huynh) {
            ppm_huynh(p, dcL, h2[L - 1], h2[L + 1]);
            if (iv == 0) ppm_limit(dcL, p, 2);
        } else {
            if (kord != 4) p.a6 = a6_of(p);
            if (kord != 6) ppm_limit(dcL, p, lmt);
        }
        pal[L] = p.al;
        par[L] = p.ar;
        pa6[L] = p.a6;
    }
    __syncthreads();
    // one output layer per lane
    const ColumnEnds ends{pe[1], pe[km + 1], q[1], q[km]};
    NoEdge none;
    for (int k = tid + 1; k <= kn; k += nt) {
        RemapState s{k, false, 0.0f, 0.0f, pe2[k], pe2[k + 1]};
        float val = 0.0f;
        bool done = false;
        if (!(s.t <= ends.pe_top) && !(s.t >= ends.pe_bot)) {
            int lo = 1, hi = km;  // first L in [1, km] with t <= pe1(L+1); exists since t < pe_bot
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s.t <= pe[mid + 1]) hi = mid; else lo = mid + 1;
            }
            for (int L = lo; L <= km && !done; ++L) {
                const LayerView v{pe[L], pe[L + 1], dp[L], q[L], Ppm{q[L], pal[L], par[L], pa6[L]}};
                done = remap_one(s, v, ends, none, val);
            }
            if (!done) {  // below the last input layer (mappm.f90:115-121); s.accum is set here
                const float delp = s.b - ends.pe_bot;
                if (delp > 0.0f) {
                    s.qsum = s.qsum + delp * ends.q_bot;
                    s.dpsum = s.dpsum + delp;
                }
                val = FV3_DIVQ(s.qsum, s.dpsum);
            }
        } else {
            val = (s.t <= ends.pe_top) ? ends.q_top : ends.q_bot;
        }
        col.q2_[(int64_t)(k - 1) * col.ld_q2] = val;
    }
}

#ifdef FV3_FAST_ARITH
#define FV3_MAPPM_CS 0  // kord > 7 always takes the exact kernels (launch_arith): none here
#else
#define FV3_MAPPM_CS 1
#endif

#if FV3_MAPPM_CS && FV3_VARIANT_KERNELS  // the solve's scratch in LDS (A/B: FV3_MAPPM_LDS)
__global__ __launch_bounds__(64) void mappm_cs_kernel(MappmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    LdsScr scr{lds + threadIdx.x, (int)blockDim.x, (a.km + 3) * (int)blockDim.x};
    DevCol col = make_col(a, c);
    mappm_cs_column(col, scr, a.km, a.kn, a.iv, a.kord);
}
#endif

#if FV3_MAPPM_CS
// NT > 0: the bottom NT edges of the solve stay in registers (mappm_cs_column), 6 NT
// fewer scratch accesses per column; the scratch keeps its full [2][km+3] shape
// PF > 0: loads run PF levels ahead in the solve, one layer ahead in the main loop
// (mappm_cs_column).  C32: buffer loads / stores at 32-bit offsets (DevColBuf / GlobalScrBuf).
template <int NT, int PF, bool C32, int KORD = 0>
__global__ __launch_bounds__(256) void mappm_cs_global_kernel(MappmArgs a)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if constexpr (C32) {
        GlobalScrBuf scr{mrsrc(a.scratch), (uint32_t)(c * 4), (uint32_t)(stride * 4),
                         (uint32_t)((a.km + 3) * stride * 4)};
        DevColBuf d = make_col_buf(a, c);
        mappm_cs_column<DevColBuf, GlobalScrBuf, NT, PF, KORD>(d, scr, a.km, a.kn, a.iv, a.kord);
    } else {
        GlobalScr scr{a.scratch + c, stride, (int64_t)(a.km + 3) * stride};
        DevCol col = make_col(a, c);
        mappm_cs_column<DevCol, GlobalScr, NT, PF>(col, scr, a.km, a.kn, a.iv, a.kord);
    }
}

// register-tail depth of the kord > 7 kernel (every depth gives the same bits).  Measured
// on MI355X (tools/ab.py, profiles/r04c_mappm_nt.log), C384 79 -> 79: at
// 884,736 columns NT = 0 / 16 / 32 / 48 take 0.89 / 0.97 / 1.12 / 1.24 ms (the registers
// cost occupancy: 60 -> 78 / 100 / 132 VGPRs, 8 -> 6 / 4 / 3 waves per SIMD, and the
// launch needs it more than the scratch bytes saved); at one rank's 110,592 columns,
// where occupancy is not the limit, 0.232 / 0.223 / 0.218 / 0.212 ms.  So the tail is
// used on small grids only.  FV3_MAPPM_CS_NT=0|16|32|48 forces a depth (A/B).
const void* cs_global_kernel(const MappmArgs& a, int64_t nlanes)
{
    const int64_t ncol = a.ncol;
    int nt = ncol < 262144 ? 48 : 0;
    // load distance (tools/ab.py; C384 79 -> 79 kord 10, buffer operations):
    // before the rolling subgrid flags (profiles/r04l_mappm_pf.log) 884,736 columns PF =
    // 0 / 2 / 4 / 8 0.909 / 0.761 / 0.798 / 0.836 ms (64-bit addresses, PF = 0: 0.871),
    // 110,592 columns (register tail) 0.224 / 0.185 / 0.182 / 0.182 ms; with them
    // (profiles/r04q_mappm_kord_ab.log) PF = 2 / 4 0.772 / 0.765 ms and 0.175 / 0.170 ms
    int pf = 4;
#if FV3_VARIANT_KERNELS
    if (const char* e = fv3::variant_env("FV3_MAPPM_CS_NT")) nt = atoi(e);
    if (const char* e = fv3::variant_env("FV3_MAPPM_CS_PF")) pf = atoi(e);
#endif
    // buffer operations at 32-bit byte offsets when every array (and the scratch) spans
    // < 4 GiB: the last column's offset plus km levels
    auto fits = [&](const fv3_layout& l, int nlev) { return fits_c32(l, ncol, nlev); };
    bool c32 = fits(a.l_pe1, a.km + 1) && fits(a.l_q1, a.km) && 4 * nlanes * 2 * (int64_t)(a.km + 3) < (1ll << 32) - 4;
    if (const char* e = fv3::variant_env("FV3_MAPPM_CS_C32")) c32 = c32 && atoi(e) != 0;
#if FV3_VARIANT_KERNELS  // the other depths and load distances (A/B)
#define FV3_CS_PF(NT_, C_)                                                        \
    switch (pf) {                                                                 \
    case 0: return (const void*)mappm_cs_global_kernel<NT_, 0, C_>;               \
    case 4: return (const void*)mappm_cs_global_kernel<NT_, 4, C_>;               \
    case 8: return (const void*)mappm_cs_global_kernel<NT_, 8, C_>;               \
    default: return (const void*)mappm_cs_global_kernel<NT_, 2, C_>;              \
    }
    if (pf != 4 || (nt != 0 && nt != 48)) {
        if (c32) {
            if (nt == 8) { FV3_CS_PF(8, true) }
            if (nt == 16) { FV3_CS_PF(16, true) }
            if (nt) { FV3_CS_PF(48, true) } else { FV3_CS_PF(0, true) }
        }
        if (nt) { FV3_CS_PF(48, false) }
        FV3_CS_PF(0, false)
    }
#undef FV3_CS_PF
#endif
    // kord 10 under the register tail at the default load distance: the column
    // specialised for it (0.170 -> 0.168 ms at 110,592 columns; on the full grid the
    // specialised build measured slower, 0.772 -> 0.806 ms at PF = 2, so it is not used
    // there; profiles/r04q_mappm_kord_ab.log).  FV3_MAPPM_CS_KORD=0: the generic column.
    const char* ke = fv3::variant_env("FV3_MAPPM_CS_KORD");
    if (c32 && nt == 48 && (a.kord == 10 || a.kord == -10) && !(ke && atoi(ke) == 0))
        return (const void*)mappm_cs_global_kernel<48, 4, true, 10>;
    if (c32) return nt ? (const void*)mappm_cs_global_kernel<48, 4, true> : (const void*)mappm_cs_global_kernel<0, 4, true>;
    return nt ? (const void*)mappm_cs_global_kernel<48, 4, false> : (const void*)mappm_cs_global_kernel<0, 4, false>;
}
#endif  // FV3_MAPPM_CS

}  // namespace

// ---- one or two fields on one column's edges (fv3_mappm_multi, the lane-split kernels) ----

// DevCol for mappm_ppm_columns<NF> (NF = 1, 2): fields f emit output k in turn, so each
// keeps its own running output pointer
template <int NF>
struct DevColN {
    const float* pe1_;
    const float* q1_[NF];
    float* q2_[NF];
    int64_t ld_pe1, ld_q1[NF], ld_q2[NF];
    EdgeCursor edge;
    __device__ __forceinline__ float pe2(int k) const { return edge.pe2(k); }
    __device__ __forceinline__ float next_edge(int k) { return edge.next_edge(k); }
    __device__ __forceinline__ float q1(int f, int k) const { return q1_[f][(int64_t)(k - 1) * ld_q1[f]]; }
    __device__ __forceinline__ float pe1(int k) const { return pe1_[(int64_t)(k - 1) * ld_pe1]; }
    __device__ __forceinline__ void emit(int f, int, float v)
    {
        *q2_[f] = v;
        q2_[f] += ld_q2[f];
    }
};

// DevColN of column c over the first NF fields of a
template <int NF>
__device__ __forceinline__ DevColN<NF> make_cols(const MappmPairArgs& a, int64_t c)
{
    DevColN<NF> d;
    d.pe1_ = a.pe1 + col_offset(a.l_pe1, c);
    d.edge.pe2_ = a.pe2 + col_offset(a.l_pe2, c);
    d.ld_pe1 = a.l_pe1.ld;
    d.edge.ld_pe2 = a.l_pe2.ld;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        d.q1_[f] = a.q1[f] + col_offset(a.l_q1[f], c);
        d.q2_[f] = a.q2[f] + col_offset(a.l_q2[f], c);
        d.ld_q1[f] = a.l_q1[f].ld;
        d.ld_q2[f] = a.l_q2[f].ld;
    }
    d.edge.kn = a.kn;
    d.edge.seek(1);
    return d;
}

#ifndef FV3_MAPPM_PAIR_CARRY
#define FV3_MAPPM_PAIR_CARRY 1  // 0: tools A/B builds
#endif
template <bool K1>
__global__ __launch_bounds__(256) void mappm_ppm_pair_kernel(MappmPairArgs a)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.ncol) return;
    DevColN<2> d = make_cols<2>(a, c);
    mappm_ppm_columns<2, DevColN<2>, FV3_MAPPM_PAIR_CARRY != 0>(d, a.km, a.kn, K1 ? 1 : a.iv, K1 ? 1 : a.kord);
}

// Small grids with one lane per column left the SIMDs short of waves (one rank's share
// of C384 at world 8, 110,592 columns: 1.7 waves per SIMD, the serial remap's latency
// unhidden).  Here each column runs on LANES = 2 or 3 lanes: lane p streams the outputs
// split_bound(p) .. split_bound(p + 1) - 1, the first from input layer 1, each later one
// from the input layer where the single pass begins its first output (mappm_multi.h,
// "two lanes per column").  A block is LANES waves over the same 64 columns, wave p the
// lanes p, so every lane of a wave is in the same phase of its column (neighbouring
// columns' remap events mostly coincide; with the shares mixed in one wave they diverge
// at every level).  A later lane finds its start layer in two rounds of loads; every lane
// checks the sortedness that the start layers rely on on the edges it streams, and after
// the block barrier the first lane re-runs the single pass on any column the checks did
// not prove (unsorted or NaN edges).  The host runs this kernel for kn >= LANES only, on
// NF = 2 fields (fv3_mappm_multi's pairs) or one (fv3_mappm_ex).
template <int NF, bool K1, int LANES>
__global__ __launch_bounds__(64 * LANES) void mappm_ppm_pair_split_kernel(MappmPairArgs a)
{
    const int iv = K1 ? 1 : a.iv, kord = K1 ? 1 : a.kord;
    __shared__ SplitCheck s_chk[LANES - 1][64];  // of the lanes after the first
    __shared__ int s_l0[LANES - 1][64];
    const int lane = threadIdx.x & 63;
    const int part = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * 64 + lane;
    const bool valid = c0 < a.ncol;
    const int64_t c = valid ? c0 : a.ncol - 1;  // spare lanes only pass the barrier
    DevColN<NF> d = make_cols<NF>(a, c);
    const int km = a.km, kn = a.kn;
    // this lane's outputs [kf, kl] and first input layer (one call site for every lane);
    // the bounds of each p are scalar arithmetic, selected per wave (as one expression of
    // `part` they are vector arithmetic: 65,536 columns, one field, 49.9 -> 50.4 us)
    int kf = 1, kl = kn;
#pragma unroll
    for (int p = 0; p < LANES; ++p)
        if (part == p) {
            kf = split_bound<LANES>(p, kn);
            kl = split_bound<LANES>(p + 1, kn) - 1;
        }
    const int Lf = part == 0 ? 1 : split_first_layer(d, km, kf);
    SplitCheck chk{1, km};
    if (valid) {
        // the output pointers and the edge cursor where the single pass has them once
        // output kf - 1 is written
        float* q2c[NF];
        for (int f = 0; f < NF; ++f) {
            q2c[f] = d.q2_[f];
            d.q2_[f] += (int64_t)(kf - 1) * d.ld_q2[f];
        }
        d.edge.seek(kf);
        mappm_ppm_columns<NF, DevColN<NF>, FV3_MAPPM_PAIR_CARRY != 0, true>(d, km, kn, iv, kord, kf, kl, Lf, &chk);
        for (int f = 0; f < NF; ++f) d.q2_[f] = q2c[f];
    }
    if (part > 0) {
        s_chk[part - 1][lane] = chk;
        s_l0[part - 1][lane] = Lf;
    }
    __syncthreads();
    if (part == 0 && valid) {
        SplitCheck chks[LANES] = {chk};
        int L0[LANES] = {1};
        for (int p = 1; p < LANES; ++p) {
            chks[p] = s_chk[p - 1][lane];
            L0[p] = s_l0[p - 1][lane];
        }
        if (!split_joins<LANES>(chks, L0, km)) {
            // the fix-up: this column's single pass, over what the lanes wrote
            d.edge.seek(1);
            mappm_ppm_columns<NF, DevColN<NF>, FV3_MAPPM_PAIR_CARRY != 0>(d, km, kn, iv, kord);
        }
    }
}

// NF fields on two or three lanes per column: 64 * lanes threads per 64 columns
template <int NF>
hipError_t launch_split(MappmPairArgs a, int lanes, hipStream_t stream)
{
    const void* kfn = pick_k1(a.iv, a.kord, [&](auto k1) {
        constexpr bool K1 = decltype(k1)::value;
        return lanes == 3 ? (const void*)mappm_ppm_pair_split_kernel<NF, K1, 3>
                          : (const void*)mappm_ppm_pair_split_kernel<NF, K1, 2>;
    });
    void* kargs[] = {&a};
    return hipLaunchKernel(kfn, dim3((unsigned)((a.ncol + 63) / 64)), dim3(64 * lanes), kargs, 0, stream);
}

int launch_mappm(MappmArgs a, hipStream_t stream)
{
    if (a.ncol == 0) return FV3_OK;
#if FV3_MAPPM_CS
    if (a.kord > 7 && !(FV3_VARIANT_KERNELS && fv3::variant_env("FV3_MAPPM_LDS"))) {
        const int block = 256;
        const int64_t grid = (a.ncol + block - 1) / block;
        FV3_HIP(hipMallocAsync((void**)&a.scratch, sizeof(float) * 2 * (size_t)(a.km + 3) * (size_t)grid * block,
                               stream));
        void* kargs[] = {&a};
        FV3_HIP(hipLaunchKernel(cs_global_kernel(a, grid * block), dim3((unsigned)grid), dim3(block), kargs, 0, stream));
        FV3_LAUNCH_CHECK();
        FV3_HIP(hipFreeAsync(a.scratch, stream));
        return FV3_OK;
    }
#endif
    if (a.kord > 7) {
#if FV3_MAPPM_CS && FV3_VARIANT_KERNELS
        const int block = 64;
        const size_t lds = sizeof(float) * 2 * (size_t)(a.km + 3) * block;
        FV3_REQUIRE(lds <= 160 * 1024, "mappm: km=%d too large for the kord>7 LDS path", a.km);
        const int64_t grid = (a.ncol + block - 1) / block;
        hipLaunchKernelGGL(mappm_cs_kernel, dim3((unsigned)grid), dim3(block), lds, stream, a);
#else
        FV3_REQUIRE_CODE(FV3_ERR_UNSUPPORTED, false, "mappm: kord > 7 runs on the exact kernels only");
#endif
    } else if (const PpmKernel kernel = ppm_kernel(1, a.ncol, a.km, a.kn); kernel == kPpmLevels) {
        const int block = a.km + 1 > 64 ? 128 : 64;
        const size_t lds = sizeof(float) * (9 * (size_t)(a.km + 2) + (size_t)(a.kn + 2));
        FV3_REQUIRE(lds <= 64 * 1024, "mappm: km=%d kn=%d too large for the level-parallel path", a.km, a.kn);
        FV3_REQUIRE(a.ncol <= 0x7fffffff, "mappm: ncol too large for the level-parallel path");
        hipLaunchKernelGGL(mappm_ppm_levels_kernel, dim3((unsigned)a.ncol), dim3(block), lds, stream, a);
    } else if (kernel == kPpmLanes1) {
        const int block = 256;
        const int64_t grid = (a.ncol + block - 1) / block;
        // q1 / pe1 by buffer loads wherever they fit 32-bit offsets (FV3_MAPPM_PPM_BUF=0:
        // 64-bit addresses, A/B)
        bool buf = fits_c32(a.l_pe1, a.ncol, a.km + 1) && fits_c32(a.l_q1, a.ncol, a.km);
        if (const char* e = fv3::variant_env("FV3_MAPPM_PPM_BUF")) buf = buf && atoi(e) != 0;
        const void* kfn = pick_k1(a.iv, a.kord, [&](auto k1) {
            constexpr bool K1 = decltype(k1)::value;
            return buf ? (const void*)mappm_ppm_kernel<K1, true> : (const void*)mappm_ppm_kernel<K1, false>;
        });
        void* kargs[] = {&a};
        FV3_HIP(hipLaunchKernel(kfn, dim3((unsigned)grid), dim3(block), kargs, 0, stream));
    } else {  // one field on two or three lanes per column
        const MappmPairArgs pa{a.pe1, a.pe2, a.l_pe1, a.l_pe2, {a.q1, nullptr}, {a.q2, nullptr}, {a.l_q1, {}},
                               {a.l_q2, {}}, a.ncol, a.km, a.kn, a.iv, a.kord};
        FV3_HIP(launch_split<1>(pa, kernel, stream));
    }
    FV3_LAUNCH_CHECK();
    return FV3_OK;
}

// a pair of fields on the streaming kord <= 7 kernels (fv3_mappm_multi), `lanes` per column
int launch_mappm_pairs(MappmPairArgs a, int lanes, hipStream_t s)
{
    if (lanes > 1) {
        FV3_HIP(launch_split<2>(a, lanes, s));
    } else {
        const int block = 256;
        const int64_t grid = (a.ncol + block - 1) / block;
        const void* kfn =
            pick_k1(a.iv, a.kord, [](auto k1) { return (const void*)mappm_ppm_pair_kernel<decltype(k1)::value>; });
        void* kargs[] = {&a};
        FV3_HIP(hipLaunchKernel(kfn, dim3((unsigned)grid), dim3(block), kargs, 0, s));
    }
    FV3_LAUNCH_CHECK();
    return FV3_OK;
}

}  // namespace FV3_ARITH_NS
}  // namespace fv3

#ifndef FV3_FAST_ARITH  // the C ABI: one definition, dispatching on the arithmetic
using fv3::MappmArgs;

namespace {
// FV3_ARITH_FAST covers the ppm_profile path (kord <= 7) only.  cs_profile (kord > 7)
// flattens a layer or switches its Huynh constraint on flags (extm, ext5, ext6,
// mappm.f90:269-288) computed from the solved edges, a discontinuous choice: 1-ulp
// changes to the edges flip it (tools/remap_fast_study.py, C384 kord 10: 7e-3 per level,
// 1 % of the values moved).  So kord > 7 always runs the exact arithmetic, and so do the
// ppm_profile calls whose interior limiter is the discontinuous lmt 2 (kord 5; kord 7
// with iv 0): fast_arith_serves, mappm_core.h.
bool use_fast(int arith, int iv, int kord) { return arith == FV3_ARITH_FAST && fv3::fast_arith_serves(iv, kord); }

int launch_arith(const MappmArgs& a, int arith, hipStream_t s)
{
    return use_fast(arith, a.iv, a.kord) ? fv3::fast::launch_mappm(a, s) : fv3::exact::launch_mappm(a, s);
}
}  // namespace

extern "C" int fv3_mappm_arith(int iv, int kord, int arith)
{
    if (arith != FV3_ARITH_EXACT && arith != FV3_ARITH_FAST) return -1;
    return use_fast(arith, iv, kord) ? FV3_ARITH_FAST : FV3_ARITH_EXACT;
}

extern "C" int fv3_mappm_ex(const float* pe1, fv3_layout pe1_l, const float* q1, fv3_layout q1_l,
                            const float* pe2, fv3_layout pe2_l, float* q2, fv3_layout q2_l,
                            int64_t ncol, int km, int kn, int iv, int kord, float ptop, int arith,
                            void* stream)
{
    (void)ptop;  // unused by the reference too (regridz.py:270)
    fv3::clear_error();
    FV3_REQUIRE(arith == FV3_ARITH_EXACT || arith == FV3_ARITH_FAST, "mappm: unknown arithmetic %d", arith);
    FV3_REQUIRE(ncol >= 0, "mappm: ncol must be >= 0 (got %lld)", (long long)ncol);
    FV3_REQUIRE(km >= 4, "mappm: km must be >= 4 (got %d)", km);
    FV3_REQUIRE(kn >= 1, "mappm: kn must be >= 1 (got %d)", kn);
    FV3_REQUIRE(ncol == 0 || (pe1 && q1 && pe2 && q2), "mappm: NULL array");
    FV3_REQUIRE(ncol == 0 || (fv3::layout_ok(pe1_l, ncol) && fv3::layout_ok(q1_l, ncol) &&
                              fv3::layout_ok(pe2_l, ncol) && fv3::layout_ok(q2_l, ncol)),
                "mappm: invalid column layout");
    FV3_REQUIRE(ncol / 256 < (int64_t)0x7fffffff, "mappm: ncol too large");
    MappmArgs a{pe1, q1, pe2, q2, pe1_l, q1_l, pe2_l, q2_l, ncol, km, kn, iv, kord, nullptr};
    return launch_arith(a, arith, (hipStream_t)stream);
}

// the f2py signature of the reference's mappm.mappm: the reference's arithmetic
extern "C" int fv3_mappm(const float* pe1, const float* q1, const float* pe2, float* q2,
                         int64_t ncol, int km, int kn, int iv, int kord, float ptop, void* stream)
{
    const fv3_layout l = fv3::plain_layout(ncol > 0 ? ncol : 1);
    return fv3_mappm_ex(pe1, l, q1, l, pe2, l, q2, l, ncol, km, kn, iv, kord, ptop, FV3_ARITH_EXACT, stream);
}

extern "C" int fv3_mappm_multi(const float* pe1, fv3_layout pe1_l, const float* const* q1, const fv3_layout* q1_l,
                               const float* pe2, fv3_layout pe2_l, float* const* q2, const fv3_layout* q2_l,
                               int n_fields, int64_t ncol, int km, int kn, int iv, int kord, float ptop, int arith,
                               void* stream)
{
    fv3::clear_error();
    FV3_REQUIRE(arith == FV3_ARITH_EXACT || arith == FV3_ARITH_FAST, "mappm: unknown arithmetic %d", arith);
    FV3_REQUIRE(n_fields >= 1 && n_fields <= 64, "mappm_multi: n_fields must be in 1..64 (got %d)", n_fields);
    FV3_REQUIRE(q1 && q1_l && q2 && q2_l, "mappm_multi: NULL field array");
    FV3_REQUIRE(ncol >= 0, "mappm: ncol must be >= 0 (got %lld)", (long long)ncol);
    FV3_REQUIRE(km >= 4, "mappm: km must be >= 4 (got %d)", km);
    FV3_REQUIRE(kn >= 1, "mappm: kn must be >= 1 (got %d)", kn);
    if (ncol == 0) return FV3_OK;
    FV3_REQUIRE(pe1 && pe2, "mappm: NULL array");
    FV3_REQUIRE(fv3::layout_ok(pe1_l, ncol) && fv3::layout_ok(pe2_l, ncol), "mappm: invalid column layout");
    for (int f = 0; f < n_fields; ++f) {
        FV3_REQUIRE(q1[f] && q2[f], "mappm_multi: NULL field %d", f);
        FV3_REQUIRE(fv3::layout_ok(q1_l[f], ncol) && fv3::layout_ok(q2_l[f], ncol),
                    "mappm_multi: invalid column layout of field %d", f);
    }
    FV3_REQUIRE(ncol / 256 < (int64_t)0x7fffffff, "mappm: ncol too large");
    const hipStream_t s = (hipStream_t)stream;
    int f = 0;
    // pairs on the streaming kord <= 7 kernels; the level-parallel (small grids) and
    // cs_profile (kord > 7) paths, and an odd last field, one field per launch
    const fv3::PpmKernel pair = kord <= 7 ? fv3::ppm_kernel(2, ncol, km, kn) : fv3::kPpmLevels;
    if (pair != fv3::kPpmLevels) {
        for (; f + 2 <= n_fields; f += 2) {
            fv3::MappmPairArgs a{pe1, pe2, pe1_l, pe2_l, {q1[f], q1[f + 1]}, {q2[f], q2[f + 1]},
                                 {q1_l[f], q1_l[f + 1]}, {q2_l[f], q2_l[f + 1]}, ncol, km, kn, iv, kord};
            const int st = use_fast(arith, iv, kord) ? fv3::fast::launch_mappm_pairs(a, pair, s)
                                                     : fv3::exact::launch_mappm_pairs(a, pair, s);
            if (st != FV3_OK) return st;
        }
    }
    for (; f < n_fields; ++f) {
        const int st = fv3_mappm_ex(pe1, pe1_l, q1[f], q1_l[f], pe2, pe2_l, q2[f], q2_l[f], ncol, km, kn, iv, kord,
                                    ptop, arith, stream);
        if (st != FV3_OK) return st;
    }
    return FV3_OK;
}
#endif  // FV3_FAST_ARITH
