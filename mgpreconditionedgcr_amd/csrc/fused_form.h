// Which form of the fused GCR apply kernels (gcr_fused.hip) an operator takes — pure arithmetic: plain values in, plain struct
// out, no HIP header — tests/cpp/fused_form_check.cpp runs it on the CPU.  The workgroup's rows and the entry size come in as arguments.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mgcr {

// rows that reach at least this far take the LDS-window kernels (MGCR_FUSED_TILE_REACH overrides it there; the one-launch step of
// gcr_stepbuild.hip leaves them those operators by this value, whatever the override)
constexpr int64_t FUSED_TILE_REACH_DEFAULT = (int64_t)1 << 15;

// the grid of red_grid's g logical workgroups: from 64 on a multiple of 8 => XCD bands
inline unsigned fused_grid(int g) { return (unsigned)(g >= 64 ? (g + 7) / 8 * 8 : g); }
// two alternating windows of a workgroup's rows + halo on both sides
inline size_t fused_window_bytes(int wg_rows, int32_t halo, size_t entry_bytes) { return 2 * (size_t)(wg_rows + 2 * halo) * entry_bytes; }

struct FusedOperator {   // what the selection reads of a CsrDev
    bool stencil;        // the kernels read the stencil view
    bool rare;           // ... in its rare-tail layout (7 common + 2 rare slots)
    int slots;           // ... of 7 or 9 kernel slots
    uint32_t near_f;
    int32_t halo_f;
    int64_t reach;
    int pat_mode;
    int32_t W;
    size_t pat_lds_bytes;   // the pattern table of a mode-1 dictionary
};
struct FusedSetup {
    bool tile_on, xr_tile_on;   // MGCR_FUSED_TILE, MGCR_XR_FUSE_TILE
    int64_t min_reach;          // MGCR_FUSED_TILE_REACH
    int wg_rows;                // RED_THREADS
    size_t entry_bytes;         // sizeof(cplx)
};

// the windowed regime: x staged per trip in an LDS window that serves slots 1..5 of the 7 common ones (step_apply_tile_kernel)
inline bool fused_windowed_regime(const FusedOperator &op, const FusedSetup &s) {
    return op.stencil && op.near_f == 0x3eu && op.halo_f > 0 && (op.rare || op.slots == 7) && s.tile_on && op.reach >= s.min_reach;
}
// ... and where the residual update may move into it (csr_xr_fusable asks this before the short-row case)
inline bool fused_xr_windowed_regime(const FusedOperator &op, const FusedSetup &s) { return fused_windowed_regime(op, s) && s.xr_tile_on; }

enum class FusedUse { Step, Init, Xr };   // csr_step_apply, csr_init_apply, csr_step_apply_xr

struct FusedForm {
    bool windowed;   // step_apply_tile_kernel & co <NS, RARE, ..>; otherwise step_apply_kernel & co <MODE, WT, ..>
    int mode;        // 0 slab, 1 / 2 dictionary, 3 stencil view, 4 stencil view with the rare tail (windowed: unused, 0)
    int ns;          // windowed: NS; otherwise WT (0: the width is a run-time value)
    bool rare;
    bool pw, carry;       // the instantiation's PW and CARRY arguments
    size_t win_bytes;     // 0 unless windowed
    size_t lds_bytes;     // the launch's dynamic LDS
    const char *error;    // Xr only: nullptr, or why there is no such kernel
};

// pw: the launch's last workgroup folds and exchanges (Step only); carried: the far slots are one step of the banded row map away
// (gcr_fused.hip tile_carry; asked for in the windowed regime only); xr_ap_ok: more than XR_TILE_APC_NDT dot streams, or the last is A p
inline FusedForm fused_form(const FusedOperator &op, const FusedSetup &s, FusedUse use, bool pw, bool carried, bool xr_ap_ok = true) {
    FusedForm f{};
    pw = pw && use == FusedUse::Step;
    if (fused_windowed_regime(op, s)) {
        f.windowed = true;
        f.rare = op.rare;
        f.ns = op.rare ? 9 : 7;
        f.win_bytes = f.lds_bytes = fused_window_bytes(s.wg_rows, op.halo_f, s.entry_bytes);
        if (use == FusedUse::Xr) {   // <7, false> with the carried far slots, nothing else
            f.carry = true;
            if (op.rare || !carried || !xr_ap_ok) f.error = "not the windowed form's case";
        } else {
            f.pw = pw;
            f.carry = carried && (op.rare || !pw);   // 7 slots: PW wins over CARRY
        }
    } else if (op.stencil) {
        f.mode = op.rare ? 4 : 3;
        f.ns = op.rare || op.slots != 7 ? 9 : 7;
        f.rare = op.rare;
        f.pw = pw;
    } else {
        f.mode = op.pat_mode == 1 || op.pat_mode == 2 ? op.pat_mode : 0;
        f.ns = op.W == 7 ? 7 : 0;
        f.lds_bytes = op.pat_lds_bytes;
        f.pw = pw;
    }
    return f;
}

}  // namespace mgcr
