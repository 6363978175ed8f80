// Host build of the scheduler's rule for what a run's second solver waits for (mdrp_amd/csrc/mdrp_schedule.h, second_solver_after) for
// tests/test_solver_order_host.py: plain C entry points, no GPU.
// g++ -O2 -std=c++17 -fPIC -shared solver_order_host.cpp -o libsolver_order_host.so
#include "../../mdrp_amd/csrc/mdrp_schedule.h"

using namespace mdrp::sched;

extern "C" {

// 1: behind k_prep, 0: behind the first chunk's solver
int so_second_solver_behind_prep(int kind, int presampled, int host_buffers, int n_chunks, int knob) {
    return second_solver_after(kind, presampled != 0, host_buffers != 0, n_chunks, knob) == SolveAfter::prep ? 1 : 0;
}
}
