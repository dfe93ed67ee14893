// TEST-ONLY host build of the product's streaming mappm (fv3net_amd/csrc/mappm_core.h).
// Lets the CPU test suite check the one-pass algorithm bit-for-bit against the
// oracle without a GPU.  Not part of the product library and never loaded by it.
//
// With -DFV3_FAST_ARITH -DFV3_EMULATE_DEVICE_RCP (and FMA contraction available, -mfma) it
// is the default arithmetic as the device rounds it: the reciprocal is the correctly
// rounded one moved by +1 / -1 ulp for a quarter of the denominators each (the device's
// v_rcp_f32 is good to 1 ulp; a function of the denominator, so equal denominators share
// one reciprocal as on the device), and div_refined takes the device's FMA refinement.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#if defined(FV3_FAST_ARITH) && defined(FV3_EMULATE_DEVICE_RCP)
static inline float fv3_emulated_rcp(float b)
{
    const float r = 1.0f / b;
    uint32_t u;
    std::memcpy(&u, &b, 4);
    const uint32_t h = (u * 2654435761u) >> 30;  // 0, 1: as rounded; 2: one ulp up; 3: one ulp down
    if (h < 2 || !std::isfinite(r) || r == 0.0f) return r;
    return h == 2 ? std::nextafterf(r, INFINITY) : std::nextafterf(r, -INFINITY);
}
#define FV3_RCP(b) fv3_emulated_rcp(b)
#define FV3_HOST_DEVICE_DIV 1
#endif
#include "../../fv3net_amd/csrc/mappm_choice.h"
#include "../../fv3net_amd/csrc/mappm_core.h"

namespace {
struct Col {
    const float *pe1_, *q1_, *pe2_;
    float* q2_;
    int64_t ncol, i;
    int kn;
    float q1(int k) const { return q1_[(int64_t)(k - 1) * ncol + i]; }
    float pe1(int k) const { return pe1_[(int64_t)(k - 1) * ncol + i]; }
    float pe2(int k) const { return pe2_[(int64_t)(k - 1) * ncol + i]; }
    void emit(int k, float v) { q2_[(int64_t)(k - 1) * ncol + i] = v; }
    float next_edge(int k) const { return (k + 1 <= kn + 1) ? pe2(k + 1) : 0.0f; }
};
struct Scr {
    std::vector<float> ev, gv;
    float& e(int k) { return ev[k]; }
    float& g(int k) { return gv[k]; }
};
}  // namespace

// whether the default arithmetic serves (iv, kord), as the product's hosts ask it
extern "C" int host_fast_arith_serves(int iv, int kord) { return fv3::fast_arith_serves(iv, kord) ? 1 : 0; }

// the kord <= 7 kernel the product's host launches (mappm_choice.h): 0 level-parallel, 1 /
// 2 / 3 lanes per column; the knobs' values as strings, NULL for unset
extern "C" int host_ppm_kernel_choice(int fields, int64_t ncol, int km, int kn, int n_cu, const char* path,
                                      const char* split, const char* split1)
{
    return fv3::ppm_kernel_choice(fields, ncol, km, kn, n_cu, fv3::PpmKnobs{path, split, split1});
}

extern "C" int host_mappm(int km, const float* pe1, const float* q1, int kn, const float* pe2,
                          float* q2, int64_t ncol, int iv, int kord)
{
    if (km < 4 || kn < 1) return -1;
    Scr scr{std::vector<float>(km + 3), std::vector<float>(km + 3)};
    for (int64_t i = 0; i < ncol; ++i) {
        Col c{pe1, q1, pe2, q2, ncol, i, kn};
        if (kord > 7)
            fv3::mappm_cs_column(c, scr, km, kn, iv, kord);
        else
            fv3::mappm_ppm_column(c, km, kn, iv, kord);
    }
    return 0;
}

// kord > 7 with the bottom `nt` edges in registers (mappm_cs_column<..., NT>), as the
// device kernel runs it: the same bits as host_mappm's all-scratch column
extern "C" int host_mappm_cs_tail(int km, const float* pe1, const float* q1, int kn, const float* pe2,
                                  float* q2, int64_t ncol, int iv, int kord, int nt)
{
    if (km < 4 || kn < 1 || kord <= 7) return -1;
    Scr scr{std::vector<float>(km + 3), std::vector<float>(km + 3)};
    for (int64_t i = 0; i < ncol; ++i) {
        Col c{pe1, q1, pe2, q2, ncol, i, kn};
        switch (nt) {
        case 8: fv3::mappm_cs_column<Col, Scr, 8>(c, scr, km, kn, iv, kord); break;
        case 16: fv3::mappm_cs_column<Col, Scr, 16>(c, scr, km, kn, iv, kord); break;
        case 32: fv3::mappm_cs_column<Col, Scr, 32>(c, scr, km, kn, iv, kord); break;
        case 48: fv3::mappm_cs_column<Col, Scr, 48>(c, scr, km, kn, iv, kord); break;
        default: return -1;
        }
    }
    return 0;
}

// kord > 7 with the loads run `pf` levels ahead (mappm_cs_column<..., NT, PF>) and the
// bottom `nt` edges in registers, as the device kernel runs it
template <int NT>
static int cs_pf(Col& c, Scr& scr, int km, int kn, int iv, int kord, int pf)
{
    switch (pf) {
    case 2: fv3::mappm_cs_column<Col, Scr, NT, 2>(c, scr, km, kn, iv, kord); return 0;
    case 4: fv3::mappm_cs_column<Col, Scr, NT, 4>(c, scr, km, kn, iv, kord); return 0;
    case 8: fv3::mappm_cs_column<Col, Scr, NT, 8>(c, scr, km, kn, iv, kord); return 0;
    default: return -1;
    }
}
extern "C" int host_mappm_cs_prefetch(int km, const float* pe1, const float* q1, int kn, const float* pe2,
                                      float* q2, int64_t ncol, int iv, int kord, int nt, int pf)
{
    if (km < 4 || kn < 1 || kord <= 7) return -1;
    Scr scr{std::vector<float>(km + 3), std::vector<float>(km + 3)};
    for (int64_t i = 0; i < ncol; ++i) {
        Col c{pe1, q1, pe2, q2, ncol, i, kn};
        const int st = nt == 0 ? cs_pf<0>(c, scr, km, kn, iv, kord, pf) : cs_pf<16>(c, scr, km, kn, iv, kord, pf);
        if (st) return st;
    }
    return 0;
}

// same through the output-driven cursor (kord <= 7), as the fused coarsen kernel uses it
extern "C" int host_mappm_cursor(int km, const float* pe1, const float* q1, int kn, const float* pe2,
                                 float* q2, int64_t ncol, int iv, int kord)
{
    if (km < 4 || kn < 1 || kord > 7) return -1;
    for (int64_t i = 0; i < ncol; ++i) {
        Col c{pe1, q1, pe2, q2, ncol, i, kn};
        fv3::mappm_ppm_column_by_output(c, km, kn, iv, kord);
    }
    return 0;
}

// the streaming column with the reference-shaped event loop (remap_layer) instead of
// remap_layer_fast: the two must agree bit for bit on every input, sorted or not
extern "C" int host_mappm_generic(int km, const float* pe1, const float* q1, int kn, const float* pe2,
                                  float* q2, int64_t ncol, int iv, int kord)
{
    if (km < 4 || kn < 1 || kord > 7) return -1;
    for (int64_t i = 0; i < ncol; ++i) {
        Col c{pe1, q1, pe2, q2, ncol, i, kn};
        fv3::mappm_ppm_column<Col, false>(c, km, kn, iv, kord);
    }
    return 0;
}

// the same column with level L + 4's loads carried one iteration ahead (CARRY: the
// device mappm kernel's build)
extern "C" int host_mappm_carry(int km, const float* pe1, const float* q1, int kn, const float* pe2,
                                float* q2, int64_t ncol, int iv, int kord)
{
    if (km < 4 || kn < 1 || kord > 7) return -1;
    for (int64_t i = 0; i < ncol; ++i) {
        Col c{pe1, q1, pe2, q2, ncol, i, kn};
        fv3::mappm_ppm_column<Col, true, true>(c, km, kn, iv, kord);
    }
    return 0;
}

// the window in register rings (RING: the fast single-field kernel's column), with CARRY
extern "C" int host_mappm_ring(int km, const float* pe1, const float* q1, int kn, const float* pe2, float* q2,
                               int64_t ncol, int iv, int kord)
{
    if (km < 4 || kn < 1 || kord > 7) return -1;
    for (int64_t i = 0; i < ncol; ++i) {
        Col c{pe1, q1, pe2, q2, ncol, i, kn};
        fv3::mappm_ppm_column<Col, true, true, true>(c, km, kn, iv, kord);
    }
    return 0;
}

// NF fields on one pressure column in one pass (mappm_multi.h), as the fused coarsen
// kernel runs them: q1 / q2 hold NF arrays [km][ncol] / [kn][ncol] back to back
#include "../../fv3net_amd/csrc/mappm_multi.h"
namespace {
struct ColN {
    const float *pe1_, *q1_, *pe2_;
    float* q2_;
    int64_t ncol, i;
    int km, kn;
    float q1(int f, int k) const { return q1_[((int64_t)f * km + (k - 1)) * ncol + i]; }
    float pe1(int k) const { return pe1_[(int64_t)(k - 1) * ncol + i]; }
    float pe2(int k) const { return pe2_[(int64_t)(k - 1) * ncol + i]; }
    void emit(int f, int k, float v) { q2_[((int64_t)f * kn + (k - 1)) * ncol + i] = v; }
    float next_edge(int k) const { return (k + 1 <= kn + 1) ? pe2(k + 1) : 0.0f; }
};
template <int NF, bool CARRY = false>
void run_n(int km, const float* pe1, const float* q1, int kn, const float* pe2, float* q2, int64_t ncol, int iv,
           int kord)
{
    for (int64_t i = 0; i < ncol; ++i) {
        ColN c{pe1, q1, pe2, q2, ncol, i, km, kn};
        fv3::mappm_ppm_columns<NF, ColN, CARRY>(c, km, kn, iv, kord);
    }
}
}  // namespace

// two fields with level L + 4's loads carried one iteration ahead (the device pair kernel)
extern "C" int host_mappm_pair_carry(int km, const float* pe1, const float* q1, int kn, const float* pe2, float* q2,
                                     int64_t ncol, int iv, int kord)
{
    if (km < 4 || kn < 1 || kord > 7) return -1;
    run_n<2, true>(km, pe1, q1, kn, pe2, q2, ncol, iv, kord);
    return 0;
}

extern "C" int host_mappm_multi(int nf, int km, const float* pe1, const float* q1, int kn, const float* pe2,
                                float* q2, int64_t ncol, int iv, int kord)
{
    if (km < 4 || kn < 1 || kord > 7) return -1;
    switch (nf) {
        case 1: run_n<1>(km, pe1, q1, kn, pe2, q2, ncol, iv, kord); return 0;
        case 2: run_n<2>(km, pe1, q1, kn, pe2, q2, ncol, iv, kord); return 0;
        case 3: run_n<3>(km, pe1, q1, kn, pe2, q2, ncol, iv, kord); return 0;
        case 4: run_n<4>(km, pe1, q1, kn, pe2, q2, ncol, iv, kord); return 0;
    }
    return -1;
}

// a column on LANES lanes (mappm_ppm_columns<NF, .., SPLIT>, the small-grid split kernel):
// the lanes one after the other between the kernel's bounds, start layers and join rule
// (mappm_multi.h), with the single-pass fix-up; kb > 0: the first split point instead of
// the kernel's; walk = 1: every later lane from layer 1
template <int NF, int LANES>
static void run_lanes(int km, const float* pe1, const float* q1, int kn, const float* pe2, float* q2, int64_t ncol,
                      int iv, int kord, int kb, int walk)
{
    for (int64_t i = 0; i < ncol; ++i) {
        ColN c{pe1, q1, pe2, q2, ncol, i, km, kn};
        if (kn < LANES) {  // the host runs a kernel of fewer lanes
            fv3::mappm_ppm_columns<NF, ColN, true>(c, km, kn, iv, kord);
            continue;
        }
        fv3::SplitCheck chk[LANES];
        int L0[LANES];
        for (int p = 0; p < LANES; ++p) {
            const int kf = (p == 1 && kb > 0) ? kb : fv3::split_bound<LANES>(p, kn);
            const int kl = (p == 0 && kb > 0) ? kb - 1 : fv3::split_bound<LANES>(p + 1, kn) - 1;
            L0[p] = (p == 0 || walk) ? 1 : fv3::split_first_layer(c, km, kf);
            chk[p] = fv3::SplitCheck{1, km};
            fv3::mappm_ppm_columns<NF, ColN, true, true>(c, km, kn, iv, kord, kf, kl, L0[p], &chk[p]);
        }
        if (!fv3::split_joins<LANES>(chk, L0, km)) fv3::mappm_ppm_columns<NF, ColN, true>(c, km, kn, iv, kord);
    }
}
// the first output of lane p of `lanes` (2 or 3), p = 0 .. lanes
extern "C" int host_split_bound(int lanes, int p, int kn)
{
    return lanes == 3 ? fv3::split_bound<3>(p, kn) : fv3::split_bound<2>(p, kn);
}
extern "C" int host_mappm_split3(int nf, int km, const float* pe1, const float* q1, int kn, const float* pe2,
                                 float* q2, int64_t ncol, int iv, int kord, int walk)
{
    if (km < 4 || kn < 1 || kord > 7) return -1;
    switch (nf) {
        case 1: run_lanes<1, 3>(km, pe1, q1, kn, pe2, q2, ncol, iv, kord, 0, walk); return 0;
        case 2: run_lanes<2, 3>(km, pe1, q1, kn, pe2, q2, ncol, iv, kord, 0, walk); return 0;
    }
    return -1;
}
extern "C" int host_mappm_split(int nf, int km, const float* pe1, const float* q1, int kn, const float* pe2,
                                float* q2, int64_t ncol, int iv, int kord, int kb, int walk)
{
    if (km < 4 || kn < 1 || kord > 7 || kb > kn || kb == 1) return -1;
    switch (nf) {
        case 1: run_lanes<1, 2>(km, pe1, q1, kn, pe2, q2, ncol, iv, kord, kb, walk); return 0;
        case 2: run_lanes<2, 2>(km, pe1, q1, kn, pe2, q2, ncol, iv, kord, kb, walk); return 0;
    }
    return -1;
}
