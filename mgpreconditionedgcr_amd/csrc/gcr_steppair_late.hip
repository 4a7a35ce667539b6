// The LATE-R pair form of a one-launch GCR step: gcr_steppair.hip's step_pair_kernel (the same body, gcr_steppair_body.h) under the
// policy that does not hold r of the thread's eight rows from the apply to the build.
// Why: the pair forms are register-bound — 128 VGPRs at 4 waves per SIMD is the whole file, A r takes 128 of the 160 KB of LDS —
// and every thread-row of a stored direction that a thread cannot keep from the pass-1 dots to the build is read from memory twice
// (4.19 MB per thread-row at 128^3, non-temporal streams: HBM).  rk[8], 32 VGPRs, is written by the apply and first read by the
// build's <r, Ap'>.  Here the apply drops the own value of its diagonal gather and the build loads r again, a plain load at the head
// of each batch: the lines the apply's gathers brought into the XCD's L2.  The registers keep 8-9 thread-rows more, of Ap_1 and Ap_2
// too (kept rows are one array, row u of Ap_j at j * 8 + u: SbPairPolicy).  Eight loads of r against eight or nine loads of Ap.
// The bits are step_pair_kernel's: the same operands in the same order and trees — the element loaded is the one the gather
// returned, nothing writes a.x during the launch (csr_step_build asks that a.x is neither xr_out nor p_out).
// Built where the trade can pay, with the next residual update, real coefficients, no shift: 3 and 4 directions and the close at 5.
// At 2 directions one row is gained (15 -> 16) for a whole pass of r, at 1 direction none: not built.
// Thread-rows kept, per form the most with which it compiles to 0 scratch, <= 128 VGPRs and 4 waves per SIMD
// (tests/test_stepbuild_pair_late_regs.py pins table and resources):
//   form               kept (Ap_0 + Ap_1 + Ap_2)   VGPRs   step_pair_kernel keeps   one row more
//   3 directions        22  (8 + 8 + 6)             128     14                       36 B of scratch per lane
//   4 directions        20  (8 + 8 + 4)             128     11                       36 B
//   the close at 5      20  (8 + 8 + 4)             128     12                       20 B
// -DMGCR_SB_PAIR_LATE_KEPT=K builds K rows in every form, -DMGCR_SB_PAIR_LATE_MORE=M the table's + M, for such a derivation.
// -DMGCR_SB_PAIR_LATE_FROM=U: thread-rows below U keep their r from the apply, the others load it again (a mixed policy: with U = 4,
// 16 VGPRs are freed instead of 32; build with a matching -DMGCR_SB_PAIR_LATE_KEPT).  0, all eight, is what is built.
#include "gcr_steppair_dev.h"

namespace mgcr {

#ifndef MGCR_SB_PAIR_LATE_KEPT
#define MGCR_SB_PAIR_LATE_KEPT -1
#endif
#ifndef MGCR_SB_PAIR_LATE_MORE
#define MGCR_SB_PAIR_LATE_MORE 0
#endif
#ifndef MGCR_SB_PAIR_LATE_FROM
#define MGCR_SB_PAIR_LATE_FROM 0
#endif
template <int NDT, bool CLOSE> constexpr bool sb_pair_late_built() { return CLOSE ? NDT == 5 : NDT == 3 || NDT == 4; }
template <int NDT, bool CLOSE> constexpr int sb_pair_late_kept() {
    if (MGCR_SB_PAIR_LATE_KEPT >= 0) return MGCR_SB_PAIR_LATE_KEPT;
    return (NDT == 3 ? 22 : 20) + MGCR_SB_PAIR_LATE_MORE;
}
// The forms the default dispatch launches (option step_build_pair_late = 1): by the rule of gcr_steppair.hip's sb_pair_form, those
// whose own kernel trace showed them faster than the form they replace — step_pair_kernel at 3 and 4 directions,
// step_keep_wide_kernel<5, true, true, true> at the close — by more than the rows' standard deviations.
template <int NDT, bool CLOSE> constexpr bool sb_pair_late_form() {
    // At 128^3, two traces each, interleaved: 3 directions 48.2 against 49.8 us (the rows' standard deviations 0.6 to 0.7 us), 4
    // directions 60.4 against 63.0 us (0.7 to 0.8), the close at 5 109.9 against 113.4 us (1.2 to 1.4): all three are handed out.
    return sb_pair_late_built<NDT, CLOSE>();
}

template <int NDT, bool CLOSE>
__global__ void __launch_bounds__(RED_THREADS, 4) step_pair_late_kernel(StepBuildArgs a) {
    using POL = SbPairPolicy<sb_pair_late_kept<NDT, CLOSE>(), true, MGCR_SB_PAIR_LATE_FROM>;
#include "gcr_steppair_body.h"
}

// 0: off | 1: the forms of sb_pair_late_form | 2: every built form (tests, traces)
static int g_sb_pair_late = -1;
static int sb_pair_late_mode() {
    if (g_sb_pair_late < 0) {
        const int64_t v = env_int64("MGCR_SB_PAIR_LATE", 1);
        g_sb_pair_late = v <= 0 ? 0 : v >= 2 ? 2 : 1;
    }
    return g_sb_pair_late;
}
int set_stepbuild_pair_late(int mode) {
    const int prev = sb_pair_late_mode();
    g_sb_pair_late = mode <= 0 ? 0 : mode >= 2 ? 2 : 1;
    return prev;
}

template <int NDT, bool CLOSE> static const void *sb_pair_late_entry(int mode) {
    if constexpr (sb_pair_late_built<NDT, CLOSE>())
        return mode == 2 || sb_pair_late_form<NDT, CLOSE>() ? (const void *)step_pair_late_kernel<NDT, CLOSE> : nullptr;
    else return nullptr;
}
const void *sb_pair_late_kernel(int nd, bool xr, bool close, bool realc) {
    const int mode = sb_pair_late_mode();
    if (mode == 0 || !stepbuild_pair_is_enabled() || !realc || !xr) return nullptr;
    if (close) return nd == 5 ? sb_pair_late_entry<5, true>(mode) : nullptr;
    return nd == 3 ? sb_pair_late_entry<3, false>(mode) : nd == 4 ? sb_pair_late_entry<4, false>(mode) : nullptr;
}

}  // namespace mgcr
