// The PAIR form of a one-launch GCR step (gcr_stepbuild.hip, gcr_stepbuild_keep_body.h): one physical workgroup of 1024 threads per
// CU — grid 256, up to 128 VGPRs, 4 waves per SIMD — carries TWO logical workgroups of the keep forms' launch, the two that ran on
// that XCD as physical workgroups p1 = ((b >> 3) << 4) | (b & 7) and p1 + 8 of its grid of 512.
// Why: the keep forms run two workgroups per CU at 64 VGPRs, of which 32-40 are the working set (stream batches, offsets,
// accumulators) and are paid per thread; of a thread's 4 rows of Ap_0 1 to 3 survive in registers from the pass-1 dots to the build,
// the others are read from memory twice.  Here a thread owns the 2 x 4 rows the two logical workgroups gave thread `tid`, holds the
// working set once, and keeps ALL eight rows of Ap_0 — and rows of Ap_1 where a form has registers left (sb_pair_kept) — across
// exchange 1.  A r of the eight rows lives in LDS (128 KB dynamic).
// The bits are the keep forms': every sum keeps its operands, its order and its tree.
//   * Per logical workgroup a thread accumulates over ITS four rows in trip order; a wave's trees run the two logical workgroups'
//     sums side by side (wave_multi_sum sums every scalar by the same tree whatever their number: reduce.h), and the waves' sums
//     are added in wave order per logical workgroup.  No row of one is added into a sum of the other.
//   * Two slots are published per exchange, two entries each written to partsA and partsR_out, indexed by LOGICAL number: nothing
//     downstream sees the pairing.  The hop-1 tasks of both logical numbers are folded here, on different waves (sp_collect).
//   * The scalar stage's writes go out once, from the physical workgroup that carries logical workgroup 0.
//   * |r|^2 of the step before is one value for everybody: folded once per physical workgroup.
// Built for real coefficients and an operator without a shift (A itself, not 1 - k A), with the next residual update: in-cycle
// steps at 1..4 stored directions and the close at 5 — the five kernels of the restart-5 headline.  Handed out by default: 2, 3 and
// 4 directions (sb_pair_form: the forms whose own trace cleared the gate).  Everything else keeps its kernel.
// Needs >= 256 CUs and 512 logical workgroups (gcr_stepbuild.hip csr_step_build asks; option step_build_pair, MGCR_SB_PAIR).
// The body is gcr_steppair_body.h, a text included into the kernel template under a compile-time policy (SbPairPolicy,
// gcr_steppair_dev.h): gcr_steppair_late.hip builds it a second time, as step_pair_late_kernel, which does not hold r between the
// apply and the build and keeps more rows instead; where that form is handed out (3 and 4 directions, the close at 5) it runs in
// place of the kernel here or of the keep form.
#include "gcr_steppair_dev.h"

namespace mgcr {

// Thread-rows kept in registers from the pass-1 dots to the build: the LAST rows pass 1 loads — it walks the directions last to
// first — i.e. the eight rows of Ap_0, then rows of Ap_1 (its first ones: the build meets them first).  Per form the most with which
// it compiles to 0 scratch, <= 128 VGPRs and 4 waves per SIMD (tests/test_stepbuild_pair_regs.py pins table and resources):
//   form                     kept (Ap_0 + Ap_1)   VGPRs   one row more
//   1 direction               8  (8 + 0)           106     (there is no other row)
//   2 directions             15  (8 + 7)           128     16 B of scratch per lane
//   3 directions             14  (8 + 6)           128     36 B
//   4 directions             11  (8 + 3)           125     8 B
//   the close at 5           12  (8 + 4)           128     20 B
// (two rows per batch of the build, eight loads per direction in flight in pass 1; with four rows per batch of the build the forms
// at 4 and 5 directions need 36 and 100 B with the eight rows of Ap_0 alone.)
// -DMGCR_SB_PAIR_KEPT=K builds K (<= 16) for every form with more than one direction, for such a derivation.
#ifndef MGCR_SB_PAIR_KEPT
#define MGCR_SB_PAIR_KEPT -1
#endif
template <int NDT, bool CLOSE> constexpr int sb_pair_kept() {
    if (NDT == 1) return SP_ROWS;
    if (MGCR_SB_PAIR_KEPT >= 0) return MGCR_SB_PAIR_KEPT;
    return NDT == 2 ? 15 : NDT == 3 ? 14 : NDT == 4 ? 11 : 12;
}
// The forms the default dispatch launches: those whose own kernel trace showed them faster than the keep form they replace by
// more than the rows' standard deviations.  -DMGCR_SB_PAIR_FORMS=1 / 0 hands out all / none, for a measurement.
#ifndef MGCR_SB_PAIR_FORMS
#define MGCR_SB_PAIR_FORMS -1
#endif
template <int NDT, bool XR, bool CLOSE> constexpr bool sb_pair_built() { return XR && (CLOSE ? NDT == 5 : NDT <= 4); }
template <int NDT, bool XR, bool CLOSE> constexpr bool sb_pair_form() {
    if (!sb_pair_built<NDT, XR, CLOSE>()) return false;
    if (MGCR_SB_PAIR_FORMS >= 0) return MGCR_SB_PAIR_FORMS != 0;
    // 2, 3 and 4 directions: 3.3 to 4.5 us faster than their keep forms at 128^3, the rows' standard deviations 0.6 to 2.2 us.  At 1
    // direction 2.0 us with standard deviations of 1.3 to 2.5 us, at the close 0.2 us with 1.2 to 1.4 us: not handed out.
    return !CLOSE && NDT >= 2;
}

template <int NDT, bool CLOSE>
__global__ void __launch_bounds__(RED_THREADS, 4) step_pair_kernel(StepBuildArgs a) {
    using POL = SbPairPolicy<sb_pair_kept<NDT, CLOSE>(), false>;   // r of the eight rows is held from the apply on
#include "gcr_steppair_body.h"
}

static EnvSwitch g_sb_pair{"MGCR_SB_PAIR"};
bool set_stepbuild_pair_enabled(bool on) { return g_sb_pair.set(on); }
bool stepbuild_pair_is_enabled() { return g_sb_pair.on(); }

template <int NDT, bool XR, bool CLOSE> static const void *sb_pair_entry() {
    if constexpr (sb_pair_form<NDT, XR, CLOSE>()) return (const void *)step_pair_kernel<NDT, CLOSE>;
    else return nullptr;
}
const void *sb_pair_kernel(int nd, bool xr, bool close, bool realc) {
    if (!g_sb_pair.on() || !realc || !xr) return nullptr;
    if (close) return nd == 5 ? sb_pair_entry<5, true, true>() : nullptr;
    switch (nd) {
        case 1: return sb_pair_entry<1, true, false>();
        case 2: return sb_pair_entry<2, true, false>();
        case 3: return sb_pair_entry<3, true, false>();
        case 4: return sb_pair_entry<4, true, false>();
        default: return nullptr;
    }
}

}  // namespace mgcr
