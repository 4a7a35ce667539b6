// The schedule of the queued batched GCR (gcr_multi.hip gcr_queue_run): nsys systems stream through `width` slots (columns) of
// one batched restarted solve.  Pure host arithmetic — plain values in, plain values out, no HIP header —
// tests/cpp/queue_plan_check.cpp runs it on the CPU against a stand-in for the device.
//
// The rules:
//   * at step 0 the systems 0 .. min(width, nsys) - 1 occupy the slots 0 .. in order;
//   * all columns share the phase of the restart cycle.  An ADMISSION POINT is a step count at which that phase is 0 (after a
//     closing step: a continuing column then holds exactly what a fresh solve holds after its start — r, P0 and A P0 in slot 0, its
//     four start sums);
//   * it is also an admission point, at once, when every slot is known to have stopped while systems still wait: the phase is then
//     reset (phase = 0, newest slot = 0, r back in its home block);
//   * at an admission point the host POLLS the columns' device states.  Every slot found stopped is RETIRED; waiting systems are
//     ADMITTED first in, first out, into the free slots in ascending slot index;
//   * the host also polls every check_every steps (and retires what it finds: a slot freed in mid-cycle waits for the boundary);
//   * without polling it knows that a column admitted at step G has stopped by G + max_iter; it polls when that makes every slot
//     known stopped;
//   * no step is launched while every slot is known stopped; the solve ends when nothing waits and every slot has been retired.
// The driver's loop:   for (;;) { if (poll_due()) { poll; polled(); retire(j) for every slot found stopped; }
//                                 admit(...); if (finished()) break; if (!any_running()) error; step(); launch the step; }
#pragma once

namespace mgcr {

constexpr int QP_MAX_WIDTH = 16;   // MV_MAX_K

struct QueueStep {
    int it;          // the launch's global step number (a column admitted at G is at its own step it - G)
    int lim;         // directions stored so far in this cycle
    int cur, nxt;    // slot of the newest direction before / after the step (nxt == 0: the residual goes to its home block)
    bool closing;    // the step closes the cycle
    bool any_last;   // some running column is at its own last step (own step == max_iter): it takes the finishing bookkeeping
    bool all_last;   // ... every running column is: the step ends after the residual update
};

struct QueuePlan {
    int width, nsys, restart, storage, max_it, check_every;
    int global = 0;      // steps launched so far
    int phase = 0;       // steps into the current restart cycle
    int cur = 0;         // slot of the newest direction
    int waiting = 0;     // first system that has not been admitted yet
    int last_check = 0, polled_at = 0;
    int sys[QP_MAX_WIDTH];        // the slot's system, -1: empty
    int admit_at[QP_MAX_WIDTH];   // the step count at which it was admitted
    long long admissions = 0;     // systems admitted after step 0
    int resets = 0;               // phase resets (every slot stopped in mid-cycle while systems waited)

    // restart, max_iter, check_every as in mgcr_gcr_param (restart >= 1); the slots of a cycle as gcr_prepare counts them
    QueuePlan(int width_, int nsys_, int restart_, int max_iter, int check_every_)
        : width(width_ < QP_MAX_WIDTH ? width_ : QP_MAX_WIDTH), nsys(nsys_), restart(restart_), storage(restart_),
          max_it(max_iter > 0 ? max_iter : 1), check_every(check_every_ > 0 ? check_every_ : 10) {
        if (max_iter >= 1 && max_iter + 1 < storage) storage = max_iter + 1;
        for (int j = 0; j < QP_MAX_WIDTH; j++) { sys[j] = -1; admit_at[j] = 0; }
    }

    bool occupied(int j) const { return sys[j] >= 0; }
    bool any_occupied() const {
        for (int j = 0; j < width; j++) if (occupied(j)) return true;
        return false;
    }
    // known without a poll: the column has run its max_iter steps
    bool past_deadline(int j) const { return occupied(j) && global >= admit_at[j] + max_it; }
    bool any_running() const {
        for (int j = 0; j < width; j++) if (occupied(j) && !past_deadline(j)) return true;
        return false;
    }
    bool poll_due() const {
        if (!any_occupied() || global == polled_at) return false;
        return phase == 0 || !any_running() || global / check_every != last_check;
    }
    void polled() { polled_at = global; last_check = global / check_every; }
    void retire(int j) { sys[j] = -1; }
    bool finished() const { return waiting >= nsys && !any_occupied(); }

    // the admissions of this point: slots[i] takes systems[i]; returns how many (0 unless the phase is 0 or no slot is occupied)
    int admit(int *slots, int *systems) {
        if (waiting >= nsys || (phase != 0 && any_occupied())) return 0;
        if (phase != 0) { phase = 0; cur = 0; resets++; }
        int m = 0;
        for (int j = 0; j < width && waiting < nsys; j++)
            if (!occupied(j)) {
                sys[j] = waiting;
                admit_at[j] = global;
                slots[m] = j;
                systems[m] = waiting;
                m++;
                waiting++;
            }
        if (global > 0) admissions += m;
        return m;
    }

    // the next lockstep step: the slot bookkeeping of the single solve's gcr_step
    QueueStep step() {
        QueueStep s;
        global++;
        phase++;
        s.it = global;
        s.lim = storage < phase ? storage : phase;
        const int next_phase = phase % restart == 0 ? 0 : phase;
        s.cur = cur;
        s.nxt = next_phase % storage;
        s.closing = next_phase == 0;
        int running = 0, last = 0;
        for (int j = 0; j < width; j++)
            if (occupied(j) && global <= admit_at[j] + max_it) {
                running++;
                if (global == admit_at[j] + max_it) last++;
            }
        s.any_last = last > 0;
        s.all_last = last > 0 && last == running;
        phase = next_phase;
        cur = s.nxt;
        return s;
    }
};

}  // namespace mgcr
