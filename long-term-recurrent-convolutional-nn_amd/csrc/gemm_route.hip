// gemm_route.hip -- launch_gemm: which engine a contraction runs on (gemm.h).  No kernel lives here.  The ladder below is tried top to bottom
// and the first rung that fits takes the launch; its name is what lrcn_debug_route reports, followed by ":<tile config>" (0 = 256 x 256,
// 1 = 256 x 128, 2 = 512 x 128) on the 8p-f8 / 8p / 8p-bg rungs and ":<K slices>" on 8p-splitk, and by nothing on the others:
//   8p-f8       e4m3 convolutions: gemm_8p.hip or nothing
//   8p          gemm_8p.hip when its grid fills the chip (or the CUs free beside the capped convolution grids)
//   8p-bg       gemm_8p.hip on few 256 x 128 tiles, for kBgMinRows..kBgMaxRows rows beside the capped convolution grids
//   skinny      gemm_skinny.hip, M <= 128 (with its own slab split-K for long K and few column tiles, not named in the route)
//   8p-splitk   gemm_8p.hip with K cut into slices
//   glds        gemm_glds.hip when its grid fills the chip
//   skinny-last gemm_skinny.hip, whatever M it accepts
//   glds-small  gemm_glds.hip on few tiles (still far ahead of gemm_nt); glds and glds-small count tiles x atomic K-slices
//   gemm_nt     gemm.hip's register-staged kernel: every other shape, f32 included
#include <cstdio>

#include "common.h"
#include "gemm.h"
#include "knob.h"

static thread_local char g_route[48] = "";
static thread_local int g_route_cfg = -1;
void gemm_debug_note_route(const char *route, int cfg) {
    if (route) {
        if (cfg >= 0) snprintf(g_route, sizeof(g_route), "%s:%d", route, cfg);
        else snprintf(g_route, sizeof(g_route), "%s", route);
    } else {
        g_route_cfg = cfg;  // tile config / slice count of the launch in flight (composed into the string by launch_gemm)
    }
}
const char *gemm_debug_last_route() { return g_route; }

// Beside the capped convolution grids a launch that fills this share of the FREE CUs in one round counts as filling the chip.
constexpr int kFree8pMinPct = 75;
// The 8p-bg rung is for the wide LSTM-side contractions (N = 4H, V), not the narrow projections.
constexpr int kBgMinCols = 512;

// workgroups gemm_8p.hip would launch for g (0: it does not take g)
static int64_t blocks_8p(const GemmArgs &g) {
    int64_t b = 0;
    return gemm_8p_config(g, &b) >= 0 ? b : 0;
}
// Beside the capped convolution grids only ~bg_cus CUs are free: a launch of many small workgroups runs in several rounds on them, one of
// few large tiles (less operand traffic per FLOP) in one.  The recurrent GEMM of the 256-row step (256 x 4000 x 1024) is 32 tiles of
// 256 x 128: one round on 32 free CUs.
static GemmArgs bg_args(const GemmArgs &g) {
    GemmArgs h = g;
    h.cfg_pref = 2;
    return h;
}
static bool bg_fits(const GemmArgs &g) {
    if (g.bg_cus <= 0 || g.a_mode != GEMM_A_PLAIN || !bg_row_window(g.M) || g.N < kBgMinCols) return false;
    const int64_t b = blocks_8p(bg_args(g));
    return b > 0 && b <= 2 * g.bg_cus;
}

static hipError_t launch_gemm_routed(hipStream_t stream, const GemmArgs &g, const char **route) {
    if (g.dtype == GEMM_T_F8) {  // e4m3: the phase-interleaved convolution kernel or nothing
        if (g.M <= 0 || !g.A || !g.B || !g.C || blocks_8p(g) == 0) return hipErrorInvalidValue;
        *route = "8p-f8";
        return launch_gemm_8p(stream, g);
    }
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || !g.A || !g.B || !g.C) return hipErrorInvalidValue;
    // LRCN_GLDS=0 turns every direct-to-LDS engine off (8p, skinny, glds), =force takes glds whenever eligible; LRCN_8P=0 turns the
    // phase-interleaved engine off, =force drops its grid threshold; LRCN_SKINNY=0 turns the skinny-M engine off; LRCN_8P_SPLITK=0 turns
    // the split-K form off, LRCN_8P_SPLITK_MIN is the fewest workgroups it is taken for.
    const char glds = knob_char("LRCN_GLDS"), p8 = knob_char("LRCN_8P");
    const bool glds_on = glds != '0', p8_on = glds_on && p8 != '0';
    const bool skinny_ok = glds_on && !knob_off("LRCN_SKINNY") && gemm_skinny_eligible(g);
    const bool splitk_on = p8_on && !knob_off("LRCN_8P_SPLITK");
    const int splitk_min = knob_int("LRCN_8P_SPLITK_MIN", 96);

    const int64_t b8 = p8_on ? blocks_8p(g) : 0;
    const bool fills_free = g.free_cus > 0 && b8 * 100 >= (int64_t)g.free_cus * kFree8pMinPct && b8 <= g.free_cus;
    if (b8 > 0 && (p8 == 'f' || b8 >= 128 || fills_free)) { *route = "8p"; return launch_gemm_8p(stream, g); }
    if (p8_on && bg_fits(g)) { *route = "8p-bg"; return launch_gemm_8p(stream, bg_args(g)); }
    if (p8_on && skinny_ok && g.M <= 128) { *route = "skinny"; return launch_gemm_skinny(stream, g); }
    int64_t bsk = 0;
    const int sk = splitk_on ? gemm_8p_splitk(g, &bsk) : 0;
    if (sk > 1 && bsk >= splitk_min) { *route = "8p-splitk"; return launch_gemm_8p(stream, g, sk); }
    const int64_t bgl = glds_on && gemm_glds_eligible(g) ? gemm_glds_blocks(g) : 0;
    if (bgl > 0 && (glds == 'f' || bgl >= 96)) { *route = "glds"; return launch_gemm_glds(stream, g); }
    if (skinny_ok) { *route = "skinny-last"; return launch_gemm_skinny(stream, g); }
    if (bgl >= 16) { *route = "glds-small"; return launch_gemm_glds(stream, g); }  // 128 < M <= 256 with too few tiles for the rungs above

    const int ce = g.dtype == GEMM_T_BF16 ? 8 : 4;
    if (((uintptr_t)g.A & 15) || ((uintptr_t)g.B & 15) || (g.ldb % ce)) return hipErrorInvalidValue;
    if (g.a_mode == GEMM_A_CONV3) {
        const int bk = g.dtype == GEMM_T_BF16 ? 64 : 32;
        if (g.Cin % bk || g.K != 9 * g.Cin || (g.H & 1) || (g.W & 1) || g.M % (g.H * g.W)) return hipErrorInvalidValue;
    } else if (g.lda % ce) {
        return hipErrorInvalidValue;
    }
    if (g.out_mode != GEMM_OUT_PLAIN && ((g.H & 1) || (g.W & 1) || g.H <= 0 || g.W <= 0)) return hipErrorInvalidValue;
    if (g.out_mode == GEMM_OUT_POOL && (g.beta || (g.M & 3))) return hipErrorInvalidValue;
    *route = "gemm_nt";
    return launch_gemm_nt(stream, g);
}

hipError_t launch_gemm(hipStream_t stream, const GemmArgs &g) {
    const char *route = "?";
    g_route_cfg = -1;
    const hipError_t e = launch_gemm_routed(stream, g, &route);
    gemm_debug_note_route(route, g_route_cfg);
    return e;
}
