// Drives the schedule of the queued batched GCR (csrc/queue_plan.h) with a stand-in for the device: system s stops after its[s]
// steps of its own.  tests/test_queue_plan.py builds this with the address and undefined-behaviour sanitizers and compares what it
// prints with the Python model of tests/queue_cases.py.
//     queue_plan_check WIDTH RESTART MAX_ITER CHECK_EVERY IT_0 IT_1 ...
// prints one "admit SYSTEM SLOT STEP" line per admission, one "retire SYSTEM SLOT STEP" line per retirement, one "reset STEP" line
// per phase reset and a last line "steps N admissions M resets R polls P last_steps L short_steps S".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "queue_plan.h"

using namespace mgcr;

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int width = atoi(argv[1]), restart = atoi(argv[2]), max_iter = atoi(argv[3]), check_every = atoi(argv[4]);
    std::vector<int> its;
    for (int a = 5; a < argc; a++) its.push_back(atoi(argv[a]));
    QueuePlan qp(width, (int)its.size(), restart, max_iter, check_every);
    long long polls = 0, last_steps = 0, short_steps = 0;
    for (long long guard = 0; guard < 10000000; guard++) {
        if (qp.poll_due()) {
            polls++;
            qp.polled();
            for (int j = 0; j < qp.width; j++)
                if (qp.occupied(j) && qp.global >= qp.admit_at[j] + its[(size_t)qp.sys[j]]) {
                    printf("retire %d %d %d\n", qp.sys[j], j, qp.global);
                    qp.retire(j);
                }
        }
        int slots[QP_MAX_WIDTH], systems[QP_MAX_WIDTH];
        const int resets = qp.resets;
        const int m = qp.admit(slots, systems);
        if (qp.resets != resets) printf("reset %d\n", qp.global);
        for (int i = 0; i < m; i++) printf("admit %d %d %d\n", systems[i], slots[i], qp.global);
        if (qp.finished()) {
            printf("steps %d admissions %lld resets %d polls %lld last_steps %lld short_steps %lld\n", qp.global, qp.admissions, qp.resets, polls,
                   last_steps, short_steps);
            return 0;
        }
        if (!qp.any_running()) { printf("stuck at %d\n", qp.global); return 1; }
        const QueueStep s = qp.step();
        if (s.lim < 1 || s.lim > qp.storage || s.cur < 0 || s.cur >= qp.storage || s.nxt < 0 || s.nxt >= qp.storage) {
            printf("slot out of range at %d\n", qp.global);
            return 1;
        }
        if (s.any_last) last_steps++;
        if (s.all_last) short_steps++;
    }
    printf("no end\n");
    return 1;
}
