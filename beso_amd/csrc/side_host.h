// Host code the side libraries share (select, scale, noise, rank, critic_fit, guide_fit and guide_tile.h): how an entry point
// refuses a call, and the goal contract of the row layouts.  Everything here has internal linkage: every library is one
// translation unit and keeps a last-error message of its own, which its `beso_*_last_error` returns (guide.hip and guide_fit.hip
// export none and return bare statuses).
#pragma once
#include "common.h"

#include <cstdio>

namespace beso_side {

static thread_local char g_error[224] = "";

template <typename... A>
static int refuse(int status, const char* fmt, A... a) {
    snprintf(g_error, sizeof(g_error), fmt, a...);
    return status;
}

static bool misaligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

struct Named {
    const char* name;
    const void* p;
    bool optional;
};

// the first NULL (unless optional) or misaligned pointer of `args`, by name
template <size_t N>
static int check_pointers(const char* fn, const Named (&args)[N]) {
    for (const Named& a : args) {
        if (!a.p && !a.optional) return refuse(BESO_ERR_BAD_ARG, "%s: %s is NULL", fn, a.name);
        if (misaligned(a.p, 4)) return refuse(BESO_ERR_BAD_ARG, "%s: %s is not 4-byte aligned", fn, a.name);
    }
    return BESO_OK;
}

// A goal is [n or 1, goal_steps >= 1, obs_dim] floats beside n samples: its last step is read, and a single row is shared by all
// samples.  Without one (goal == NULL) goal_steps and goal_rows are both 0.
struct GoalRows {
    long long stride, off;      // floats between two samples' goals (0: one shared goal) and to step goal_steps - 1

    static bool valid(const void* goal, int goal_steps, int goal_rows, int n) {
        return goal ? goal_steps >= 1 && (goal_rows == n || goal_rows == 1) : goal_steps == 0 && goal_rows == 0;
    }

    GoalRows(const void* goal, int goal_steps, int goal_rows, int n, int obs_dim)
        : stride(goal && goal_rows == n && n > 1 ? (long long)goal_steps * obs_dim : 0),
          off(goal ? (long long)(goal_steps - 1) * obs_dim : 0) {}
};

}  // namespace beso_side
