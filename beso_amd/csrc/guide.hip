// The guide gradient of classifier-guided sampling (include/beso_guide.h; reference k_diffusion/classifier_free_sampler.py:
// 56-90): libbeso_guide.so.  The kernel and its host call are guide_tile.h's, here over rows [state | pred | goal]; the rows with
// the noise-level column are guide_fit.hip's (libbeso_guidefit.so).
#include "guide_tile.h"
#include "../../include/beso_guide.h"

using namespace beso_guide;

extern "C" int beso_guide_supported(const beso_mlp_dims* dims, int obs_dim, int act_dim, int use_goal) {
    return check_guide(dims, obs_dim, act_dim, use_goal, 0);
}

extern "C" int beso_guide_apply(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* state,
                                const float* goal, const float* pred, const float* sigma, int B, int T, int state_steps,
                                int goal_steps, int goal_rows, int obs_dim, int act_dim, float lam, float* out, void* stream) {
    return guide_apply<false>(params, n_params, dims, state, goal, pred, sigma, nullptr, B, T, state_steps, goal_steps, goal_rows,
                              obs_dim, act_dim, lam, out, stream);
}
