// Runs the form selection of the fused GCR apply launchers (csrc/fused_form.h) on hand-made operators and prints one line
// per case; tests/test_fused_form.py builds this with the address and undefined-behaviour sanitizers and compares the lines
// with the table of forms written out by hand.
#include <cstdio>

#include "fused_form.h"

using namespace mgcr;

static const FusedSetup SETUP{true, true, FUSED_TILE_REACH_DEFAULT, 1024, 16};

// a 7-slot stencil view in the windowed regime: near slots 1..5, halo 64, rows reaching exactly the threshold.  (A stencil view
// sits on a mode-1 dictionary: its pattern table's bytes must not reach a stencil launch.)
static FusedOperator sten7() { return FusedOperator{true, false, 7, 0x3eu, 64, FUSED_TILE_REACH_DEFAULT, 1, 7, 1400}; }
static FusedOperator rare(FusedOperator op) { op.rare = true; op.slots = 9; return op; }
static FusedOperator near_by(FusedOperator op) { op.reach = 4096; return op; }
static FusedOperator stored(int pat_mode, int32_t W) { return FusedOperator{false, false, 0, 0, 0, 4096, pat_mode, W, pat_mode == 1 ? (size_t)1400 : 0}; }

static void show(const char *use_name, const char *name, const FusedOperator &op, bool pw = false, bool carried = false, bool xr_ap_ok = true,
                 const FusedSetup &s = SETUP) {
    const FusedUse use = use_name[0] == 's' ? FusedUse::Step : use_name[0] == 'i' ? FusedUse::Init : FusedUse::Xr;
    const FusedForm f = fused_form(op, s, use, pw, carried, xr_ap_ok);
    printf("%s %s ", use_name, name);
    if (f.error) { printf("error=%s\n", f.error); return; }
    if (f.windowed) printf("tile<%d,%d>", f.ns, (int)f.rare);
    else printf("plain<%d,%d>", f.mode, f.ns);
    printf(" pw=%d carry=%d win=%zu lds=%zu\n", (int)f.pw, (int)f.carry, f.win_bytes, f.lds_bytes);
}

int main() {
    // ---- the windowed rows -------------------------------------------------------------------------------------------
    for (int c = 0; c < 4; c++) {
        static const char *names[4] = {"tile-rare", "tile-rare-carried", "tile-rare-pw", "tile-rare-pw-carried"};
        show("step", names[c], rare(sten7()), (c & 2) != 0, (c & 1) != 0);
    }
    for (int c = 0; c < 4; c++) {
        static const char *names[4] = {"tile-7", "tile-7-carried", "tile-7-pw", "tile-7-pw-carried"};
        show("step", names[c], sten7(), (c & 2) != 0, (c & 1) != 0);
    }
    show("init", "tile-rare", rare(sten7()));
    show("init", "tile-rare-carried", rare(sten7()), false, true);
    show("init", "tile-7", sten7());
    show("init", "tile-7-carried", sten7(), false, true);
    show("init", "tile-7-carried-pw-asked", sten7(), true, true);
    show("xr", "tile-rare", rare(sten7()));
    show("xr", "tile-rare-carried", rare(sten7()), false, true);
    show("xr", "tile-7", sten7());
    show("xr", "tile-7-carried", sten7(), false, true);
    show("xr", "tile-7-carried-ap-elsewhere", sten7(), false, true, false);
    // ---- stencil view outside the regime, dictionary, slab: both columns (and the init apply) ------------------------------
    static const char *uses[3] = {"step", "xr", "init"};
    for (const char *u : uses) {
        FusedOperator nine = near_by(sten7());
        nine.slots = 9;
        show(u, "sten-rare", near_by(rare(sten7())));
        show(u, "sten-7", near_by(sten7()));
        show(u, "sten-9", nine);
        show(u, "dict1-w7", stored(1, 7));
        show(u, "dict1-w5", stored(1, 5));
        show(u, "dict2-w7", stored(2, 7));
        show(u, "dict2-w27", stored(2, 27));
        show(u, "slab-w7", stored(0, 7));
        show(u, "slab-w8", stored(0, 8));
    }
    show("step", "sten-rare-pw", near_by(rare(sten7())), true);
    show("step", "sten-7-pw-carried-asked", near_by(sten7()), true, true);
    show("step", "dict1-w7-pw", stored(1, 7), true);
    show("xr", "slab-w7-pw-asked", stored(0, 7), true);
    // ---- the regime's boundary -----------------------------------------------------------------------------------------
    {
        FusedOperator op = sten7();
        op.reach = FUSED_TILE_REACH_DEFAULT - 1;
        show("step", "reach-below", op);
        show("step", "reach-equal", sten7());
        op = sten7(); op.halo_f = 0;
        show("step", "halo-0", op);
        op = sten7(); op.near_f = 0x3cu;
        show("step", "near-0x3c", op);
        op = sten7(); op.slots = 9;
        show("step", "nine-common", op);
        op = sten7(); op.halo_f = 256;
        show("step", "halo-256", op);
        FusedSetup off = SETUP;
        off.tile_on = false;
        show("step", "tile-off", sten7(), false, true, true, off);
        show("step", "tile-off-rare", rare(sten7()), false, false, true, off);
        show("xr", "tile-off", sten7(), false, false, true, off);
        FusedSetup low = SETUP;
        low.min_reach = 1024;
        show("step", "min-reach-1024", near_by(sten7()), false, false, true, low);
        FusedSetup noxr = SETUP;
        noxr.xr_tile_on = false;
        printf("regime windowed %d %d %d\n", (int)fused_windowed_regime(sten7(), SETUP), (int)fused_windowed_regime(near_by(sten7()), SETUP),
               (int)fused_windowed_regime(sten7(), off));
        printf("regime xr-windowed %d %d %d\n", (int)fused_xr_windowed_regime(sten7(), SETUP), (int)fused_xr_windowed_regime(sten7(), noxr),
               (int)fused_xr_windowed_regime(near_by(sten7()), SETUP));
        show("xr", "xr-switch-off-launch", sten7(), false, true, true, noxr);   // the launch does not ask the switch: csr_xr_fusable does
    }
    printf("grid padded %u %u %u %u %u\n", fused_grid(1), fused_grid(63), fused_grid(64), fused_grid(65), fused_grid(512));
    printf("reach default %lld\n", (long long)FUSED_TILE_REACH_DEFAULT);
    return 0;
}
