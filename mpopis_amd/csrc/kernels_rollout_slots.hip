// kernels_rollout_slots.hip -- the per-slot-env twins of the car rollout kernels (mpopis_set_env_params_slots / mpopis_set_tracks):
// the kernel and launcher templates of kernels_rollout.hip instantiated with SENV = true, and launch_car_rollout_slots, which launch_rollout calls
// for a handle whose slots carry their own env.  A translation unit of its own so that the two halves compile side by side.
#if defined(MPOPIS_ROLL_PROF) || defined(MPOPIS_PATH_STATS)
#error "the dev builds instrument kernels_rollout.hip only"
#endif
#define MPOPIS_ROLLOUT_SLOT_TWINS
#include "kernels_rollout.hip"
