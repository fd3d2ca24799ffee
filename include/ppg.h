/*
 * ppg.h -- C ABI of libppg_hip.so: a batched Predator-Prey-Grass environment
 * whose per-step transition runs as hand-written HIP on MI355X (gfx950).
 *
 * The reference (doesburg11/PredPreyGrass) is pure Python and has no FFI; this
 * is the boundary a maintainer would bind with ctypes to put
 * the HIP path behind the reference's own class
 *   predpreygrass/non_evolutionary/base_environment/predpreygrass_rllib_env.py
 * ("BASE" below).  Each entry point names the reference code it replaces.
 *
 * Conventions
 *  - extern "C", POD structs, fixed-width ints, no torch / C++ types.
 *  - every function returns 0 on success or a negative PPG_E* code and never
 *    throws; ppg_last_error() gives the message for the last failure.
 *  - all device buffers are allocated and owned by the caller (PyTorch-ROCm
 *    tensors); the library borrows the raw pointers for the handle's lifetime
 *    and never frees them.  Library-owned scratch is freed by ppg_destroy().
 *  - all work is asynchronous on the caller's HIP stream (`stream` is a
 *    hipStream_t passed as void*, e.g. torch.cuda.current_stream().cuda_stream).
 *  - one handle belongs to one device and one host thread.
 *
 * State layout (one "row" = one agent slot, kept in the order of the dict that
 * the reference's step() returns, per type):
 *   rows [0, pred_capacity)                       predators
 *   rows [pred_capacity, pred_capacity+prey_cap)  prey
 * Within a type the rows are [survivors in self.agents order..., newborns of
 * the last call in birth order...]; agents that died in the last call keep
 * their row (flag PPG_ROW_DIED) until the next call, exactly like
 * self.agents / _pending_removal in the reference (BASE:222-225,383).
 */
#ifndef PPG_H
#define PPG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPG_ABI_VERSION 5

/* error codes */
#define PPG_OK 0
#define PPG_EINVAL (-1)   /* bad argument / unsupported configuration */
#define PPG_ENOMEM (-2)
#define PPG_EHIP (-3)     /* a HIP runtime call failed */
#define PPG_ENODEV (-4)   /* no usable gfx950 device */

/* row_flags bits (uint8 per row) */
#define PPG_ROW_DIED 0x01u     /* terminations[agent] == True in the last call (BASE:289,332) */
#define PPG_ROW_OWNS 0x02u     /* grid[type, pos] currently holds this agent's energy */
#define PPG_ROW_NEWBORN 0x04u  /* created by the last call (BASE:396-414) */
#define PPG_ROW_ATE 0x08u      /* agent in self.agents_just_ate (BASE:319,362) */
#define PPG_ROW_TRUNC 0x10u    /* truncations[agent] == True in the last call (BASE:232) */
#define PPG_ROW_GRID_E0 0x20u  /* second generation: grid[type, pos] still shows the full initial energy written at birth
                                * (RQ:760) although the agent holds initial_energy * reproduction_energy_efficiency */

/* env_state words (int32 per env) */
#define PPG_ENV_WORDS 20
#define PPG_ENV_N_PRED_ROWS 0   /* rows in use incl. agents that died in the last call */
#define PPG_ENV_N_PREY_ROWS 1
#define PPG_ENV_N_PRED_NEW 2    /* trailing rows that are newborns of the last call */
#define PPG_ENV_N_PREY_NEW 3
#define PPG_ENV_NEXT_PRED_ID 4  /* _next_predator_idx */
#define PPG_ENV_NEXT_PREY_ID 5  /* _next_prey_idx */
#define PPG_ENV_STEP 6          /* current_step */
#define PPG_ENV_N_PRED_ALIVE 7  /* current_num_predators */
#define PPG_ENV_N_PREY_ALIVE 8  /* current_num_prey */
#define PPG_ENV_FLAGS 9
#define PPG_ENV_STATUS 10       /* sticky anomaly bits, see PPG_STATUS_* */
#define PPG_ENV_EPISODE 11
#define PPG_ENV_FALLBACK_SPAWNS 12 /* count of BASE:759-764 events this episode */
#define PPG_ENV_CALLS 13        /* step calls served (diagnostic) */
#define PPG_ENV_OBS_PRED 14     /* predator observations written so far (wraps; for bandwidth accounting) */
#define PPG_ENV_OBS_PREY 15     /* prey observations written so far */
#define PPG_ENV_NEXT_PRED_ID_T2 16 /* second generation: _next_idx[("predator", 2)] (words 4/5 hold type 1) */
#define PPG_ENV_NEXT_PREY_ID_T2 17 /* _next_idx[("prey", 2)] */
#define PPG_ENV_DRAWS 18        /* second generation: uniforms the last call consumed (RQ:701,708) */

/* env_state[PPG_ENV_FLAGS] bits */
#define PPG_ENVF_TERM_ALL 0x01   /* terminations["__all__"] of the last call (BASE:466) */
#define PPG_ENVF_TRUNC_ALL 0x02  /* truncations["__all__"] of the last call (BASE:236) */
#define PPG_ENVF_DONE 0x04       /* episode over: the next auto-reset call resets */
#define PPG_ENVF_WAS_RESET 0x08  /* the last call was a reset, not a transition */
#define PPG_ENVF_LIST_IS_ROW_ORDER 0x10 /* self.agents == row order, not yet sorted (after reset, BASE:143) */

/* env_state[PPG_ENV_STATUS] bits */
#define PPG_STATUS_PRED_OVERFLOW 0x01  /* a birth was dropped: predator rows exhausted */
#define PPG_STATUS_PREY_OVERFLOW 0x02
#define PPG_STATUS_FALLBACK_SPAWN 0x04 /* BASE:759-764 reached (reference is non-deterministic there) */
#define PPG_STATUS_FAILED_SPAWN 0x08   /* BASE:766 reached (reference raises TypeError) */
#define PPG_STATUS_BAD_ACTION 0x10     /* action outside -1..8 (reference: KeyError at BASE:502) */
#define PPG_STATUS_KICK_OVERFLOW 0x20  /* more than 15 kickback rewards for one agent in one step (not representable) */
#define PPG_STATUS_UNIFORMS_DRY 0x40   /* ppg_step_uniforms: an env needed more uniforms than were supplied */

/* ppg_step flags */
#define PPG_STEP_RANDOM_ACTIONS 0x1u /* ignore `actions`; draw uniform actions with Philox4x32-10 on device */
#define PPG_STEP_AUTO_RESET 0x2u     /* envs whose last call ended the episode are reset instead of stepped */

#define PPG_ACTION_NONE (-1) /* agent absent from the action dict: no decay, no move (BASE:244,259) */

/* The config dict of the reference (BASE:20-61; defaults CFG = config_env.py:1-38)
 * plus the capacities of this implementation. */

typedef struct ppg_config {
    int32_t abi_version;          /* PPG_ABI_VERSION */
    int32_t grid_size;            /* BASE:53, >= 2; bounded by 64 KiB of LDS per wavefront (about 80 with 7x7/9x9 windows) */
    int32_t predator_obs_range;   /* BASE:55, 1..15 */
    int32_t prey_obs_range;       /* BASE:56, 1..15 */
    int32_t max_steps;            /* BASE:26 */
    int32_t n_possible_predators; /* BASE:44, <= 999999 */
    int32_t n_possible_prey;      /* BASE:45, <= 999999 */
    int32_t n_initial_predators;  /* BASE:46 */
    int32_t n_initial_prey;       /* BASE:47 */
    int32_t n_grass;              /* BASE:59 */
    int32_t pred_capacity;        /* predator rows per env: 64, or 128 (one wave per env: no multi-wave or cooperative plan, no
                                   * drive channels, no policy kernels; prey_capacity 128 or 256) */
    int32_t prey_capacity;        /* prey rows per env: 64, 128 or 256 */
    int32_t grass_capacity;       /* >= n_grass, multiple of 64 */
    int32_t obs_dtype;            /* 0: float64 (bit-exact with the reference), 1: float32, 2: bfloat16 (the float64 value rounded to
                                   * float32, then to bfloat16, both to nearest even: compact rows for ppg_policy_act, which stages them
                                   * without conversion -- same logits as from the float64 rows, a quarter of the bytes) */
    double reward_predator_catch_prey;  /* BASE:29 */
    double reward_prey_eat_grass;       /* BASE:30 */
    double reward_predator_step;        /* BASE:31 */
    double reward_prey_step;            /* BASE:32 */
    double penalty_prey_caught;         /* BASE:33 */
    double reproduction_reward_predator;/* BASE:34 */
    double reproduction_reward_prey;    /* BASE:35 */
    double energy_loss_per_step_predator; /* BASE:38 */
    double energy_loss_per_step_prey;     /* BASE:39 */
    double predator_creation_energy_threshold; /* BASE:40 */
    double prey_creation_energy_threshold;     /* BASE:41 */
    double initial_energy_predator;     /* BASE:49 */
    double initial_energy_prey;         /* BASE:50 */
    double initial_energy_grass;        /* BASE:60 (also the regrowth cap, BASE:254) */
    double energy_gain_per_step_grass;  /* BASE:61 */
    /* seasonal grass regrowth (base_environment_seasonal/predpreygrass_rllib_env.py:63-66,224-234,268-271):
     * gain x high for season_length_steps steps, x low for the next, repeating; <= 0 disables (base env) */
    int32_t season_length_steps;
    double season_high_multiplier;
    double season_low_multiplier;
    /* rewards: 0 = base env (BASE:288,322,328,341,365,375,409,438); 1 = net energy delta of the step
     * (project_reward_shaping/base_environment_dense_rewards/predpreygrass_rllib_env.py:242-245,291-292,328-329,440-449);
     * 2 = the same plus the reproduction reward for a parent (.../base_environment_dense_rewards_additive:470) */
    int32_t reward_mode;
    /* kickback variant (project_reward_shaping/base_environment_sparse_rewards_plus_kickback/predpreygrass_rllib_env.py
     * :48-52,86-91,325,364,434,439-449): a grandparent that is still alive is rewarded every time its child reproduces */
    int32_t kickback;                   /* 0 = base env */
    double kickback_reward_predator;
    double kickback_reward_prey;
    /* drive-conditioned variant (drive_conditioned_environment/predpreygrass_rllib_env.py, "DRV"): n_drive[species] extra
     * observation channels, each filled with one per-agent scalar (DRV:54-89,551-616); both 0 = base env.  The observation
     * tensors then have 4 + n_drive[0] (predators) / 4 + n_drive[1] (prey) channels. */
    int32_t n_drive[2];                 /* <= 4 each */
    int32_t drive_kind[2][4];           /* PPG_DRIVE_* per channel, in the order of the reference's *_drive_channels lists */
    double hunger_safe_energy[2];       /* DRV:76-77 */
    double prey_opportunity_normalizer;    /* DRV:78 */
    double predator_danger_normalizer;     /* DRV:79-82 */
    double grass_opportunity_normalizer;   /* DRV:83-86 */
} ppg_config;

#define PPG_DRIVE_HUNGER_PRESSURE 0          /* clip01(1 - energy / hunger_safe_energy), DRV:591-593 */
#define PPG_DRIVE_REPRODUCTIVE_READINESS 1   /* clip01(energy / creation threshold), DRV:595-599 */
#define PPG_DRIVE_PREY_OPPORTUNITY 2         /* clip01(np.sum(window prey channel) / normalizer), DRV:601-602 */
#define PPG_DRIVE_PREDATOR_DANGER 3          /* DRV:604-605 */
#define PPG_DRIVE_GRASS_OPPORTUNITY 4        /* DRV:607-608 */

/* Caller-owned device buffers.  B = batch, S = pred_capacity + prey_capacity,
 * NG = grass_capacity, Rp/Rq = predator/prey obs range. */
typedef struct ppg_buffers {
    uint16_t *row_xy;      /* [B,S]  (x << 8) | y          agent_positions (BASE:111) */
    double *row_energy;    /* [B,S]                        agent_energies (BASE:116) */
    int32_t *row_id;       /* [B,S]  k of "predator_k"/"prey_k" (BASE:71-72) */
    uint32_t *row_key;     /* [B,S]  ppg_lexkey(row_id): order of list.sort() on the id strings (BASE:468) */
    double *row_cumrew;    /* [B,S]                        cumulative_rewards (BASE:63) */
    uint8_t *row_flags;    /* [B,S]  PPG_ROW_* */
    double *row_reward;    /* [B,S]  rewards[agent] of the last call */
    int32_t *env_state;    /* [B,PPG_ENV_WORDS] */
    uint64_t *env_seed;    /* [B]    Philox key of each env (reset placement, random actions, spawn fallback) */
    uint16_t *grass_xy;    /* [B,NG] grass_positions (BASE:114), static after reset */
    double *grass_energy;  /* [B,NG] grass_energies (BASE:117) */
    void *obs_pred;        /* [B,pred_capacity,4,Rp,Rp] float64|float32: observations (BASE:511-526) */
    void *obs_prey;        /* [B,prey_capacity,4,Rq,Rq] */
    int32_t *row_parent;   /* [B,S]  id of the agent's (same-type) parent, -1 = none: agent_parent of the kickback variant */
    int32_t *row_lastrep;  /* [B,S]  second generation: agent_last_reproduction (RQ:115,737,999); may be NULL for ppg_create */
    uint32_t *wall_bits;   /* [B,W]  walls variant: bit (x*G + y) of env b's W = ceil(G*G/32) words set = wall cell (WO:210-250);
                            *        written by the caller, never by the library; NULL unless ppg_config_gen2.walls */
    uint8_t *row_info;     /* [B,S]  walls variant: 0 = the agent did not go through the movement phase of the last call,
                            *        else 1 + move_blocked_reason (PPG_MOVE_*); NULL unless ppg_config_gen2.walls */
} ppg_buffers;

/* move_blocked_reason of the walls variant (WO:466-488), as row_info - 1 */
#define PPG_MOVE_FREE 0
#define PPG_MOVE_WALL 1
#define PPG_MOVE_OCCUPIED 2
#define PPG_MOVE_CORNER_CUT 3
#define PPG_MOVE_LOS 4

/* ---- second generation ("RQ" = predpreygrass/non_evolutionary/red_queen/predpreygrass_rllib_env.py; the same step
 * as walls_occlusion/predpreygrass_rllib_env.py without walls and line of sight) ------------------------------
 * Two agent types per species ("type_<t>_<species>_<k>"), pools in the order reset() creates them:
 * 0 type_1_predator, 1 type_2_predator, 2 type_1_prey, 3 type_2_prey.
 * row_id  = creation_number << 17 | (type - 1) << 16 | k      (creation_number: 0,1,2,... over all agents of the
 *           episode = insertion order of the reference's agent_positions dict, RQ:584-586)
 * row_key = (type - 1) * 1771561 + ppg_lexkey(k)              (order of list.sort() on the id strings, RQ:270)
 * Observations are what the reference returns (float32 grid, RQ:137-139,352-358): use obs_dtype 1. */
typedef struct ppg_config_gen2 {
    int32_t abi_version;
    int32_t grid_size;            /* RQ:70 */
    int32_t predator_obs_range;   /* RQ:72 */
    int32_t prey_obs_range;       /* RQ:73 */
    int32_t max_steps;            /* RQ:36 */
    int32_t n_possible[4];        /* RQ:56-59, pool order; each <= 65535, sum <= 32767 */
    int32_t n_initial[4];         /* RQ:61-64 */
    int32_t n_grass;              /* RQ:76 */
    int32_t pred_capacity;        /* 64, or 128 without walls (one wave per env, prey_capacity 128 or 256: see ppg_config) */
    int32_t prey_capacity;        /* 64, 128 or 256 */
    int32_t grass_capacity;
    int32_t obs_dtype;            /* 0: float64, 1: float32 (the reference's dtype), 2: bfloat16, 3: bfloat16 cells (see ppg_config) */
    int32_t type_1_action_range;  /* RQ:85: odd, 1..7 */
    int32_t type_2_action_range;  /* RQ:86: odd, 1..7 (ignored when no type-2 agent can exist) */
    int32_t reproduction_cooldown_steps; /* RQ:696 */
    /* type-specific values, index = type - 1 (_get_type_specific, RQ:1099-1106) */
    double reward_predator_catch_prey[2];
    double reward_prey_eat_grass[2];
    double reward_predator_step[2];
    double reward_prey_step[2];
    double penalty_prey_caught[2];
    double reproduction_reward_predator[2];
    double reproduction_reward_prey[2];
    double energy_loss_per_step_predator;      /* RQ:50 */
    double energy_loss_per_step_prey;          /* RQ:51 */
    double predator_creation_energy_threshold; /* RQ:52 */
    double prey_creation_energy_threshold;     /* RQ:53 */
    double initial_energy_predator;            /* RQ:66 */
    double initial_energy_prey;                /* RQ:67 */
    double initial_energy_grass;               /* RQ:77 */
    double energy_gain_per_step_grass;         /* RQ:78 */
    double move_energy_cost_factor;            /* RQ:305: cost = distance * factor * energy */
    double max_energy_gain_per_prey;           /* RQ:598 (INFINITY = no cap) */
    double max_energy_gain_per_grass;          /* RQ:665 */
    double max_energy_predator;                /* RQ:605 */
    double max_energy_prey;                    /* RQ:672 */
    double max_energy_grass;                   /* RQ:510 */
    double energy_transfer_efficiency;         /* RQ:599,666 */
    double reproduction_energy_efficiency;     /* RQ:754,840 */
    double reproduction_chance_predator;       /* RQ:700-701 */
    double reproduction_chance_prey;
    double mutation_rate_predator;             /* RQ:81,708 */
    double mutation_rate_prey;                 /* RQ:82,793 */
    /* "WO" = walls_occlusion/predpreygrass_rllib_env.py: the same env plus static walls.  walls != 0 selects it:
     * observation channel 0 shows the walls inside the window (WO:536-541) instead of the out-of-grid mask, a move into a
     * wall cell is refused (WO:469-471), ppg_buffers.wall_bits / row_info are used, the observation tensors have
     * 4 + include_visibility_channel channels. */
    int32_t walls;
    int32_t include_visibility_channel;        /* WO:104: last channel = line-of-sight mask (WO:577-598) */
    int32_t respect_los_for_movement;          /* WO:106: no corner cutting, no moves through walls (WO:475-488) */
    int32_t mask_observation_with_visibility;  /* WO:111: channels 1-3 multiplied by the mask (WO:591-594) */
} ppg_config_gen2;

typedef struct ppg_handle ppg_handle;

int ppg_abi_version(void);

/* Validates cfg and binds the buffers.  Replaces PredPreyGrass.__init__ (BASE:18-127). */
int ppg_create(const ppg_config *cfg, int32_t batch, int32_t device, const ppg_buffers *bufs, ppg_handle **out);
int ppg_destroy(ppg_handle *h);
/* The buffers the handle was created with (borrowed device pointers; the caller keeps owning them): what a binding that did
 * not allocate them itself needs to find observations, row tables and the status words. */
int ppg_get_buffers(const ppg_handle *h, ppg_buffers *out);

/* Second generation: replaces PredPreyGrass.__init__ of the red_queen env (RQ:15-86).  bufs->row_lastrep is required.
 * The handle works with ppg_reset / ppg_observe / ppg_step / ppg_step_ordered / ppg_step_many / ppg_export_grid
 * (reproduction uniforms from Philox, keyed like the random actions) and with ppg_step_uniforms; with ppg_rollout on a cooperative
 * four-wave plan (no walls). */
int ppg_create_gen2(const ppg_config_gen2 *cfg, int32_t batch, int32_t device, const ppg_buffers *bufs, ppg_handle **out);

/* reset() (BASE:129-217) for every env: unique random placement (Philox
 * Fisher-Yates keyed by env_seed -- distributionally, not bitwise, the
 * reference's PCG64 + set-order placement), initial energies, observations.
 * seeds: optional device pointer [B]; copied into env_seed first.  episode is
 * the Philox episode counter to start from (normally 0). */
int ppg_reset(ppg_handle *h, const uint64_t *seeds, uint32_t episode, void *stream);

/* reset() (BASE:129-217) of every env with a GIVEN placement -- the `const ppg_init_state*` form of ppg_reset: what
 * the reference's reset(seed) produces once its cells are known (its PCG64 + set-order placement is captured input, not arithmetic:
 * predpreygrass_amd.placement.reference_placement re-does it on the host).  HOST arrays, cells as (x << 8) | y:
 * predators / prey in id order (agent i of its species gets id i and initial_energy_*), grass patches in patch order
 * (initial_energy_grass each).  grid[type, cell] = energy in id order, so of several agents of one species on a cell the last one
 * owns it (BASE:190-200).  Writes the row tables, the grass table and the env words, then computes the observations (one
 * ppg_observe launch); env_seed is left alone (it keys the device-side random actions).  Base-family handles. */
typedef struct ppg_init_state {
    const uint16_t *pred_xy;   /* [B][n_initial_predators] */
    const uint16_t *prey_xy;   /* [B][n_initial_prey] */
    const uint16_t *grass_xy;  /* [B][n_grass], unique within an env */
    uint32_t episode;          /* Philox episode counter to start from (normally 0) */
    uint32_t reserved_;
} ppg_init_state;
int ppg_reset_from_state(ppg_handle *h, const ppg_init_state *init, void *stream);

/* Observations for all live rows from the state currently in the buffers
 * (reset() tail BASE:215; _get_observation BASE:511; used after the host wrote
 * a captured placement or restored a snapshot, BASE:788-804). */
int ppg_observe(ppg_handle *h, void *stream);

/* step(action_dict) (BASE:219-473) for every env.
 * actions: device int8 [B,S], indexed by the row an agent had in the previous
 * call's output (PPG_ACTION_NONE = not in the dict); may be NULL with
 * PPG_STEP_RANDOM_ACTIONS.  The movement phase applies actions in row order,
 * which is the order of the previous observation dict (RLlib's protocol). */
int ppg_step(ppg_handle *h, const int8_t *actions, uint32_t flags, void *stream);

/* n_steps transitions in ONE launch -- exactly what n_steps calls of ppg_step would do, each step writing its observations / rewards /
 * flags / tables to the same buffers -- for action sources that live on the device: the uniform random policy
 * (PPG_STEP_RANDOM_ACTIONS) or an open-loop action tape `actions` = device int8 [n_steps,B,S].  Bit-identical to n_steps ppg_step calls.
 * On a handle whose wave plan is cooperative (a full GPU of 25x25 grids: the default) it runs the fused form of the cooperative step
 * kernel: a workgroup's envs never interact with any other workgroup's, so the workgroups simply run on from step to step at their
 * own pace -- no launch boundary at which everybody computes and nobody stores -- and ONE launch stream reaches 61 us per 4096-env
 * step where per-step launches need three sub-batches in flight for 66-71 (profiles/EXPERIMENTS.md, round 3).  On other handles (small batches,
 * 64x64 grids) it is the round-1 one-wave-per-env loop, which is SLOWER than per-step launches and kept only as a diagnostic.  Base
 * family without the kickback / drive variants; second-generation handles (ppg_create_gen2, no walls) on a cooperative four-wave plan
 * only (PPG_EINVAL otherwise), reproduction uniforms from the device's Philox streams as in ppg_step. */
int ppg_rollout(ppg_handle *h, int32_t n_steps, const int8_t *actions, uint32_t flags, void *stream);

/* Same, for an action dict whose iteration order differs from the previous observation dict
 * (the order matters in the reference: movement and the decay writes are applied in dict order,
 * BASE:244,259).  act_rank: device uint8 [B,S]; for every row with an action, its position among
 * the acting agents OF ITS TYPE (0..n-1, a permutation).  NULL == row order (ppg_step). */
int ppg_step_ordered(ppg_handle *h, const int8_t *actions, const uint8_t *act_rank, uint32_t flags, void *stream);

/* Second generation only: step(action_dict) (RQ:197-299) with the values `self.rng.random()` returns supplied by the
 * caller.  uniforms: device double [B, uniforms_per_env]; env b consumes its row front to back, one value for every
 * agent past its cooldown (chance gate, RQ:701) plus one more for each of those that passes the gate with enough energy
 * (mutation, RQ:708), in self.agents order.  env_state[PPG_ENV_DRAWS] reports how many were used;
 * PPG_STATUS_UNIFORMS_DRY is raised if the row was too short.  act_rank as in ppg_step_ordered (NULL = row order). */
int ppg_step_uniforms(ppg_handle *h, const int8_t *actions, const uint8_t *act_rank, const double *uniforms,
                      int32_t uniforms_per_env, uint32_t flags, void *stream);

/* ppg_step for n handles (sub-batches of one GPU's envs), handle k on streams[k], in one host call.
 * actions may be NULL (with PPG_STEP_RANDOM_ACTIONS) or an array of n device pointers. */
int ppg_step_many(ppg_handle *const *handles, int32_t n, const int8_t *const *actions, uint32_t flags,
                  void *const *streams);

/* Scheduling hint: this handle's launches overlap with launches of other handles on the same GPU (sub-batches on other
 * streams); envs_in_flight = envs of all of them together (default: the handle's own batch).  Used to choose between the
 * one-wave-per-env step kernel and the four- / eight-waves-per-env ones (wave 0 steps, all waves write the final observations),
 * which are faster while the GPU is not full: eight up to 512 envs in flight, four up to about 3072 or when LDS admits at most
 * 4 envs per CU. */
int ppg_set_envs_in_flight(ppg_handle *h, int32_t envs_in_flight);

/* Scheduling override (tests, A/B tools): which step kernel ppg_step launches for this handle.  waves = wavefronts per workgroup
 * (0 = back to the automatic choice; 1, 2, 4, 8, 16), helper_min_rows = helper wavefronts only stay for envs with at least that
 * many agent rows, coop_envs = envs sharing one workgroup (cooperative kernels: every wave of the workgroup runs one env's
 * transition, then all of them write all the workgroup's observations; 0 = one env per workgroup).  Combinations a variant has
 * no kernel for fall back to the nearest one it has.  Results never depend on the plan -- the GPU tests compare them bit for
 * bit.  The plan is fixed here, at ppg_create and at ppg_set_envs_in_flight: ppg_step itself reads no environment variables. */
int ppg_set_wave_plan(ppg_handle *h, int32_t waves, int32_t helper_min_rows, int32_t coop_envs);
int ppg_get_wave_plan(const ppg_handle *h, int32_t *waves, int32_t *helper_min_rows, int32_t *coop_envs);

/* Walls variant: tell the library that the caller has (re)written wall_bits.  It recomputes, for every cell of every env, the
 * line-of-sight mask over the observation window (one HIP launch; library-owned [B, G*G, words] in HBM) -- from then on
 * observations read a few mask words per agent instead of walking one Bresenham line per window cell (WO:492-525, 577-589).
 * Results are identical with or without it as long as it is called after every change of wall_bits (ppg_import_state does).
 * It also copies the bitmaps to the host and WAITS for the stream: when every env's bitmap equals env 0's (one wall layout for the
 * batch) all envs read env 0's masks from then on (a few KB that stay in L2). */
int ppg_walls_changed(ppg_handle *h, void *stream);

/* Scheduling only, results are unaffected: recompute the order in which the handle's envs are assigned to workgroups --
 * envs with many agent rows (much observation data to write) first, so that the load is spread evenly over the CUs.
 * Stream-ordered like a step (one small launch: a counting sort in LDS, any batch size); populations drift slowly, calling it
 * every few dozen steps is enough (bench.py: every 64).  The order is used by every later launch of the handle. */
int ppg_rebalance(ppg_handle *h, void *stream);

/* Cache policy only, results are unaffected (the same bits): the cooperative step kernels write the observation rows of envs with
 * index >= n with non-temporal stores, which do not displace what is resident in the 256 MiB Infinity Cache, so that the rows of envs
 * 0 .. n-1 -- always the same addresses -- are rewritten in place there from step to step instead of going to HBM.  ppg_rebalance
 * computes n on the device: the largest count of leading envs whose rows in use fit budget * batch / envs in flight
 * (ppg_set_envs_in_flight; budget: 160 MiB, environment variable PPG_RESIDENT_BYTES read at ppg_create, 0 = off -- ppg_rebalance
 * then leaves the word alone).  A handle that was never rebalanced, or whose envs in flight all fit, writes every row with plain
 * stores.  ppg_set_resident_envs writes n directly (tests, A/B runs; it waits for the stream) until the next ppg_rebalance;
 * ppg_get_resident_envs reads it back (batch if it was never written; waits for the stream).  ppg_rollout's fused kernels, the
 * walls variant and the one-env-per-workgroup kernels ignore it. */
int ppg_set_resident_envs(ppg_handle *h, int32_t n, void *stream);
int ppg_get_resident_envs(ppg_handle *h, int32_t *n, void *stream);

/* grid_world_state (BASE:124): dense float64 [B,4,G,G] rebuilt from the rows. */
int ppg_export_grid(ppg_handle *h, double *grid_out, void *stream);

/* ---- snapshot of one env (get_state_snapshot / restore_state_snapshot, BASE:768-804; consumers
 * evaluate_ppo_from_checkpoint_debug.py:164-182) ------------------------------------------------------------
 * A snapshot is a versioned POD image in HOST memory: struct ppg_state_header followed by env `env`'s slice of every
 * state tensor of ppg_buffers in the order of ppg_state_field[] below (row tables, env words, Philox key + episode,
 * grass table, and for the variants row_parent / row_lastrep / row_info / wall_bits).  Observations, rewards of the last
 * call included, are NOT part of it: ppg_observe() recomputes the observations of the live rows after an import.
 * Both calls are synchronous: they enqueue the copies on `stream` and wait for them. */
#define PPG_STATE_MAGIC 0x53475050u /* "PPGS" */
#define PPG_STATE_VERSION 1u
typedef struct ppg_state_header {
    uint32_t magic, version;
    uint32_t bytes;            /* size of the whole image incl. this header */
    uint32_t gen2, walls;      /* which ppg_create* made the handle */
    uint32_t grid_size, pred_capacity, prey_capacity, grass_capacity, n_wall_words;
    uint32_t reserved[6];
} ppg_state_header;

/* bytes an image of one env of this handle takes */
uint64_t ppg_state_bytes(const ppg_handle *h);
/* env `env` -> blob (host memory, *size bytes available; on return *size = bytes written).  blob == NULL: only report the size. */
int ppg_export_state(ppg_handle *h, int32_t env, void *blob, uint64_t *size, void *stream);
/* blob -> env `env`; the image must come from a handle with the same geometry (checked through the header). */
int ppg_import_state(ppg_handle *h, int32_t env, const void *blob, uint64_t size, void *stream);

/* ---- packed observation image (ONE collective per step for the returned observation dict) --------
 * ppg_pack writes what the last call of the n handles (sub-batches of one GPU, envs concatenated in handle order)
 * returned -- env words, per-row ids / rewards / flags and the observations of the rows IN USE, compacted -- into one
 * contiguous device buffer that a single all-gather (RCCL) can move.  Layout, every section 16-byte aligned, in this order:
 *   ppg_pack_header | env_state int32[n_envs][PPG_ENV_WORDS] | row_off uint32[n_envs][2] (exclusive prefix sums of the
 *   predator / prey row counts) | id_pred int32[Np] | id_prey int32[Nq] | reward_pred double[Np] | reward_prey double[Nq] |
 *   flags_pred uint8[Np] | flags_prey uint8[Nq] | obs_pred elem[Np][blk_pred] | obs_prey elem[Nq][blk_prey]
 * (Np / Nq = rows in use over all envs, env-major, row order = dict order).  If the image does not fit in `capacity`
 * bytes the header has overflow = 1 and bytes_used = the size it needs; the row sections are then not written. */
#define PPG_PACK_MAGIC 0x4B475050u /* "PPGK" */
#define PPG_PACK_VERSION 1u
#define PPG_PACK_F32 0x1u /* float64 observations travel as float32 (observations that already are float32 are copied) */
#define PPG_PACK_NO_OBS 0x2u /* no observation sections (header blk_pred = blk_prey = 0): env words, row offsets, ids, rewards and
                              * flags only, 13 bytes per agent row + 88 per env -- what a learner or logger needs from a rollout whose
                              * policy runs next to the env (ppg_policy_act): ~2 MB per 4096-env shard and step instead of ~370 MB */
#define PPG_PACK_MAX_HANDLES 8
typedef struct ppg_pack_header {
    uint32_t magic, version;
    uint32_t n_envs, n_pred_rows, n_prey_rows;
    uint32_t obs_elem_bytes;       /* 4 or 8 */
    uint32_t blk_pred, blk_prey;   /* elements per observation: channels * R * R */
    uint64_t bytes_used, capacity;
    uint32_t overflow, env_words;
    uint32_t reserved[2];
} ppg_pack_header;                 /* 64 bytes */

/* size of an image with the given totals (host helper; h gives the geometry) */
uint64_t ppg_pack_bytes(const ppg_handle *h, int32_t n_envs, int64_t n_pred_rows, int64_t n_prey_rows, uint32_t flags);
/* asynchronous on `stream`, which the caller has ordered behind the handles' last step (two small launches) */
int ppg_pack(ppg_handle *const *handles, int32_t n, void *out, uint64_t capacity, uint32_t flags, void *stream);

/* ---- host view of the last call (what PredPreyGrass.step() hands back, BASE:219,456-473) -------------------------
 * The reference's step() returns Python dicts of one env; the dict classes of this library rebuild them from the row
 * tables and the observation rows IN USE.  ppg_fetch brings exactly that to the host in ONE image -- one gather launch
 * into a library-owned staging buffer, one asynchronous copy into `host` (pinned memory keeps it asynchronous), one
 * stream synchronisation -- for the envs [env0, env0 + n_envs) of a handle:
 *   ppg_fetch_header | n_envs x record | observation sections, env by env
 * record (record_bytes each) = the env's slice of every state tensor in the order of the state image (ppg_export_state):
 *   row_xy u16[S] | row_energy f64[S] | row_id i32[S] | row_key i32[S] | row_cumrew f64[S] | row_flags u8[S] |
 *   row_reward f64[S] | row_parent i32[S] | env_state i32[PPG_ENV_WORDS] | env_seed u64 | grass_xy u16[NG] |
 *   grass_energy f64[NG] | second generation: row_lastrep i32[S] | walls: row_info u8[S], wall_bits u32[n_wall_words]
 * each slice padded to 8 bytes, the record to 16.  Observation section of an env = its predator blocks in use
 * (env word PPG_ENV_N_PRED_ROWS of them, blk_pred_bytes each), padded to 16 bytes, then its prey blocks likewise, in the
 * handle's observation dtype.  If the image does not fit `capacity`, header.overflow = 1, bytes_used = the size it needs
 * and only header + records are valid.  Synchronous: the image is complete when the call returns. */
#define PPG_FETCH_MAGIC 0x46475050u /* "PPGF" */
#define PPG_FETCH_VERSION 1u
typedef struct ppg_fetch_header {
    uint32_t magic, version;
    uint32_t env0, n_envs;
    uint32_t record_bytes;
    uint32_t blk_pred_bytes, blk_prey_bytes;
    uint32_t overflow;
    uint64_t bytes_used, capacity;
    uint32_t reserved[4];
} ppg_fetch_header;                /* 64 bytes */

/* size of an image of n_envs envs with the given row totals (upper bound: every run of blocks padded to 16 bytes) */
uint64_t ppg_fetch_bytes(const ppg_handle *h, int32_t n_envs, int64_t n_pred_rows, int64_t n_prey_rows);
int ppg_fetch(ppg_handle *h, int32_t env0, int32_t n_envs, void *host, uint64_t capacity, void *stream);

/* ---- rows across calls (trajectories from the tensor API) -----------------------------------------------------------
 * Row order is the API, and it changes with every call: the rows of agents that died are dropped, the newborns of the last call
 * are merged into sorted position, new newborns are appended.  ppg_link joins the row_id tables of two outputs on the device
 * (one launch, one wavefront per env; csrc/ppg_link.h) against a library-owned snapshot of what the PREVIOUS ppg_link call of this
 * handle saw (ids [B,S], PPG_ENV_EPISODE [B], row counts [B,2]; allocated on the first call, freed by ppg_destroy):
 *   prev_row[b][r]  for a row r in use now: the row its agent had in the snapshot, or -1
 *   next_row[b][r]  for a row r in use in the snapshot: the row its agent has now, or -1 if it is gone
 * Both are caller-owned device int16 [B,S]; either may be NULL.  Indices are absolute positions in the [B,S] tables (predators
 * 0 .. pred_capacity-1, prey from pred_capacity), so gather(x, 1, max(idx, 0)) works directly.  Rows not in use hold -1.  The
 * call then overwrites the snapshot with the current ids, episode and counts.  -1 cases:
 *   - a row flagged PPG_ROW_NEWBORN has prev_row -1 (a row flagged PPG_ROW_DIED is still in use: it links to where the agent
 *     stood, and carries the terminal reward; next_row of a row that had DIED in the snapshot is -1).  This also holds with NO
 *     step between two ppg_link calls: every other row in use then links to itself, a row still flagged NEWBORN has -1 in both
 *     maps;
 *   - an env whose PPG_ENV_EPISODE differs from the snapshot's -- an auto-reset between the two calls -- has -1 everywhere: ids
 *     restart with every episode ((species, row_id) is unique WITHIN one: csrc/ppg_link.h);
 *   - the first ppg_link of a handle, and the first after ppg_reset / ppg_reset_from_state (all envs) or after ppg_import_state
 *     (the imported env only), give -1: those calls invalidate the snapshot on the host.  State written straight into the
 *     tensors is not seen: call ppg_link once and discard the result.
 * Any number of steps, or a ppg_rollout of K steps, may lie between two calls: the maps are then the K-step maps (agents born AND
 * dead in between appear in neither).  Asynchronous on `stream`, ordered behind the handle's last step on that stream. */
int ppg_link(ppg_handle *h, int16_t *prev_row, int16_t *next_row, void *stream);

/* ---- one step into trajectory buffers ---------------------------------------------------------------------------------
 * ppg_record is ppg_link(h, prev_row, next_row, stream) PLUS the stores that keep the output of the handle's last call as step t
 * of a trajectory, in the same launch (one wavefront per env; csrc/ppg_record.h).  It IS a link call: it uses and overwrites the
 * same library-owned snapshot, prev_row / next_row (either may be NULL) are written exactly as by ppg_link, every -1 case above
 * holds, and ppg_link and ppg_record calls may be mixed freely.  The buffers of ppg_record_buffers are caller-owned, contiguous
 * device tensors [horizon,B,S] (B and S are the handle's), the inputs of ppg_backward.  For every row r of every env b:
 *   next_row[t-1][b][r] = the link's next_row[b][r]                      -- only if t > 0
 *   next_row[t][b][r]   = -1
 *   reward[t][b][r]     = the bits of row_reward[b][r]                    -- all S rows, in use or not
 *   in_use[t][b][r]     = r < pred_capacity ? r < n_pred_rows : r - pred_capacity < n_prey_rows          (uint8 0 / 1)
 *   terminated[t][b][r] = in_use && (row_flags[b][r] & PPG_ROW_DIED)      truncated: likewise with PPG_ROW_TRUNC
 * and no other element of the buffers is touched.  The step index t:
 *   flags == 0                      t = step.  A step outside [0, horizon) is PPG_EINVAL.
 *   PPG_RECORD_STEP_ON_DEVICE       `step` is the address of an int32 in DEVICE memory that the kernel reads when it runs: a step
 *                                   captured into a hipGraph (ppg_step + ppg_record + an increment of that word) can be replayed.
 *                                   If the word is outside [0, horizon) when the kernel runs, the launch behaves exactly like
 *                                   ppg_link(h, prev_row, next_row): the snapshot advances, no buffer is written -- a replay past
 *                                   the horizon cannot write out of bounds (the word becomes an index only after that check).
 * PPG_EINVAL (text in ppg_last_error, nothing is launched, the snapshot is untouched): buf NULL, one of the five buffers NULL,
 * horizon < 1, a host step outside [0, horizon), a NULL device address, unknown flag bits.  Asynchronous on `stream`, ordered
 * behind the handle's last step on that stream. */
typedef struct ppg_record_buffers {
    int32_t horizon;       /* T */
    double *reward;        /* [T,B,S] */
    uint8_t *in_use, *terminated, *truncated;   /* [T,B,S], 0 / 1 (what a bool tensor holds) */
    int16_t *next_row;     /* [T,B,S] */
} ppg_record_buffers;
#define PPG_RECORD_STEP_ON_DEVICE 0x1u
int ppg_record(ppg_handle *h, const ppg_record_buffers *buf, uint64_t step, uint32_t flags, int16_t *prev_row, int16_t *next_row,
               void *stream);

/* ---- observations and actions into a compact per-species sample store ------------------------------------------------
 * ppg_record_obs appends the observation rows IN USE of the handle's last call -- exactly ppg_record's in_use: the first
 * n_pred_rows / n_prey_rows rows of each species' region, each count taken as min(max(n, 0), capacity of the region) -- as step t to
 * two caller-owned dense stores, one per species (s = 0 predators, 1 prey), and writes down which (t, b, r) every slot holds.  The slot
 * number is then a learner's sample index: obs[s][k] is dense, returns / advantages / values are one index_select by sample[s][k].
 * Two launches (one wavefront, then one wavefront per env; csrc/ppg_obs_store.h), no atomics.  All tensors of ppg_obs_store are
 * contiguous device memory; B, S and the observation geometry are the handle's.
 *   Order    envs in ascending b, within an env the rows in use in ascending r.  With c_s = cursor[s] before the call (taken as
 *            min(max(c_s, 0), capacity[s])) and off_s[b] = the rows of species s in use in the envs < b, row r of env b gets slot
 *            k = c_s + off_s[b] + r (prey: r - pred_capacity in place of r).
 *   Stores   if k < capacity[s]:  obs[s][k]    = the row's blk_s elements, byte for byte (PPG_OBS_F32 on a float64 handle: every element
 *                                                rounded to float32, to nearest even)
 *                                 sample[s][k] = (t * B + b) * S + r
 *                                 action[s][k] = PPG_ACTION_UNSET          (if action[] is given)
 *                                 slot[t][b][r] = k
 *   Overflow if k >= capacity[s] the row is dropped whole: slot[t][b][r] = -1 and no element of the store is written for it.  After
 *            the call cursor[s] = min(c_s + total_s, capacity[s]) and cursor[2 + s] has grown by the number of rows dropped.  A
 *            capacity of 0 drops every row.  No value read from device memory (cursor, the per-env bases, slot[t-1]) becomes an
 *            address before it was compared with capacity[s].
 *   Rows not in use get slot[t][b][r] = -1: all B * S entries of slot[t] are written, and no other element of slot is.
 *   Actions  (actions != NULL, action[] given, t > 0)  `actions` is the [B,S] int8 tensor the handle's last step was given: it is
 *            indexed by the rows of the PREVIOUS output, whose observations it answers.  For every (b, r) with
 *            k = slot[t-1][b][r] and 0 <= k < capacity[s] (k is read from memory: it is range-checked, a word outside is ignored)
 *            the call writes action[s][k] = actions[b][r].  So action[s][k] is the action taken FROM the observation in slot k,
 *            written one call later; the slots of the last recorded step keep PPG_ACTION_UNSET.  An env whose call t was an
 *            auto-reset gets the bytes stored all the same: the step ignored them, and its rows of step t - 1 are terminal.  With
 *            device-drawn random actions (PPG_STEP_RANDOM_ACTIONS) there is no tensor to pass: actions = NULL.
 *   Step     flags without PPG_OBS_STEP_ON_DEVICE: t = step; a step outside [0, horizon) is PPG_EINVAL.  With it `step` is the
 *            address of an int32 in DEVICE memory that both kernels read when they run (as PPG_RECORD_STEP_ON_DEVICE; pass the same
 *            word to ppg_record and count it up behind both); if the word is outside [0, horizon) NOTHING is written, the cursor
 *            included: a replay past the horizon stores nothing.
 * PPG_EINVAL (text in ppg_last_error, nothing is launched): st NULL; slot, cursor, sample[s] or obs[s] NULL; horizon < 1; a
 * capacity < 0 or above INT32_MAX (slot holds int32); horizon * B * S above INT32_MAX (sample holds int32); only one of the two
 * action[] pointers set; PPG_OBS_F32 on a handle whose observations are narrower than float32 (bfloat16); a host step outside
 * [0, horizon); a NULL device address; unknown flag bits.
 * The call does not touch the link snapshot and no env state, and may stand before or behind the ppg_record of the same step.  The
 * per-env slot bases live in a library-owned [B,2] int64 scratch (allocated by the first call, freed by ppg_destroy).  Asynchronous
 * on `stream`, ordered behind the handle's last step on that stream. */
#define PPG_ACTION_UNSET (-128)          /* action[k] of a slot whose action has not been recorded (yet) */
typedef struct ppg_obs_store {
    int32_t  horizon;        /* T */
    void    *obs[2];         /* [capacity[s], blk_s] elements; s = 0 predators, 1 prey; blk_s = the elements of one observation
                                row of the handle (channels * R_s * R_s, the handle's own geometry: base, gen-2, walls, drive) */
    int64_t  capacity[2];    /* rows each store can hold */
    int32_t *sample[2];      /* [capacity[s]]  (t * B + b) * S + r of the row held in slot k */
    int8_t  *action[2];      /* [capacity[s]]  may both be NULL */
    int32_t *slot;           /* [T,B,S]  slot of row r of step t in its species' store, or -1 */
    int64_t *cursor;         /* device int64 [4]: rows stored {pred, prey}, rows dropped {pred, prey} */
} ppg_obs_store;
#define PPG_OBS_STEP_ON_DEVICE 0x1u   /* as PPG_RECORD_STEP_ON_DEVICE */
#define PPG_OBS_F32            0x2u   /* float64 observations are stored as float32 (as PPG_PACK_F32); other dtypes copied */
int ppg_record_obs(ppg_handle *h, const ppg_obs_store *st, uint64_t step, uint32_t flags, const int8_t *actions, void *stream);

/* ---- the behaviour policy's log-probabilities into the sample store ---------------------------------------------------
 * ppg_record_logp writes, for every sample that ppg_record_obs stored as step t, what the policy that acted on it thought: the
 * log-probability of the action taken (PPO's ratio), the entropy, and on request the logits themselves (the distribution inputs of a
 * KL term).  The logits are the float32 tensors ppg_policy_act wrote for the handle's CURRENT output -- logits_pred / logits_prey,
 * [B * rows_s, n_actions[s]], env-major in row order: with off_s[b] = the rows of species s in use in the envs < b, row j of species s
 * in env b is logits row i = off_s[b] + j.  They cannot be recomputed later from the stored observations: the kernels of
 * ppg_policy_act round to bf16 between layers, and the actions were drawn from THESE numbers.  Either logits pointer may be NULL: that
 * species is skipped (like a NULL policy in ppg_policy_act) and none of its tensors is touched.  `actions` is the [B,S] int8 tensor
 * ppg_policy_act filled (required).  Two launches (one wavefront, then one wavefront per env and one lane per row;
 * csrc/ppg_logp.h), no atomics, nothing read back.  All tensors are contiguous device memory; B, S and the row counts are the handle's.
 *   Rows     species s, row j < n_s(b) -- the rows in use exactly as ppg_record_obs takes them: min(max(n, 0), rows of the region) --
 *            with r = j (prey: pred_capacity + j), a = actions[b][r], k = st->slot[t][b][r], A = n_actions[s].
 *   Stores   if 0 <= k < st->capacity[s] (k is read from memory: it is range-checked before it becomes an address):
 *              logp[s][k]        = log-softmax of logits row i at a; quiet NaN if a is outside [0, A) (PPG_ACTION_UNSET, -1 ...): a
 *                                  is compared with [0, A) and never used as an index
 *              entropy[s][k]     = - sum p log p of the row               (if entropy[] is given)
 *              dist[s][k][0..A)  = the row's A logits, bit for bit          (if dist[] is given)
 *            Rows not in use, rows the store dropped (slot -1) and slot words outside the capacity write nothing, and no other
 *            element of any tensor is written; st->obs, sample, action, slot and cursor are not written at all (cursor, obs, sample
 *            and action are not even read and may be NULL).
 *   Numbers  the float32 logits l are widened to float64; m = max l, e_a = exp(l_a - m), s = sum e_a in ascending a,
 *            logp = (l_a - m) - log(s), entropy = log(s) - (sum e_a (l_a - m)) / s, each rounded ONCE to float32 at the store; no fused
 *            multiply-add.  A logit of -inf is a masked action: legal while one logit of the row is finite, it contributes exactly 0 to
 *            both sums (the term is skipped, never formed as 0 * inf) and its own logp is -inf.  A row without a finite maximum (all
 *            -inf, a +inf) and a row that holds a NaN give NaN in logp and entropy; dist is copied all the same.
 *   Step     t is the recorded step whose observations the logits were computed from: the handle's current output, which ppg_record /
 *            ppg_record_obs stored as step t.  The call stands BEHIND ppg_policy_act and IN FRONT of the next ppg_step (the env state
 *            words must still be those ppg_record_obs saw).  flags without PPG_LOGP_STEP_ON_DEVICE: t = step; a step outside
 *            [0, horizon) is PPG_EINVAL.  With it `step` is the address of the int32 in DEVICE memory that ppg_record /
 *            ppg_record_obs take and that is counted up behind them: it already names the NEXT step, so t = word - 1, read by both
 *            kernels when they run; if t is outside [0, horizon) -- nothing recorded yet, or a replay past the horizon -- NOTHING is
 *            written (t becomes an index only after that check).
 * PPG_EINVAL (text in ppg_last_error, nothing is launched): st, out or actions NULL; st->slot NULL; logp[s] NULL for a species whose
 * logits are given; only one of entropy[0] / entropy[1] or of dist[0] / dist[1] set; n_actions[s] outside 1..32 for a species whose
 * logits are given; horizon < 1, a capacity < 0 or above INT32_MAX, horizon * B * S above INT32_MAX (what ppg_record_obs refuses); a
 * host step outside [0, horizon); a NULL device address; unknown flag bits.  With both logits NULL the call checks its arguments and
 * launches nothing.
 * One handle per call: sub-batches that share one ppg_policy_act call share its logits tensor, which this call cannot split -- give
 * each sub-batch its own act call.  The call touches no env state and not the link snapshot.  The per-env row offsets live in a
 * library-owned [B,2] int32 scratch (allocated by the first call, freed by ppg_destroy).  Asynchronous on `stream`, ordered behind
 * the ppg_policy_act that wrote the logits on that stream. */
typedef struct ppg_logp_store {
    float  *logp[2];      /* [capacity[s]]; required for a species whose logits are given */
    float  *entropy[2];   /* [capacity[s]]; both NULL or both set */
    float  *dist[2];      /* [capacity[s], n_actions[s]]; both NULL or both set */
    int32_t n_actions[2]; /* 1..32 */
} ppg_logp_store;
#define PPG_LOGP_STEP_ON_DEVICE 0x1u
int ppg_record_logp(ppg_handle *h, const ppg_obs_store *st, const ppg_logp_store *out, uint64_t step, uint32_t flags,
                    const float *logits_pred, const float *logits_prey, const int8_t *actions, void *stream);

/* ---- returns and advantages over a recorded horizon ------------------------------------------------------------------
 * What a learner does with the maps of ppg_link: the backward recursions over n_steps recorded calls, discounted returns G and
 * generalised advantages A, in ONE launch (one wavefront per env, the values of step t + 1 in LDS; csrc/ppg_backward.h).  All
 * tensors are caller-owned, contiguous device [n_steps,B,S] (B and S are the handle's): reward float64, next_row int16 (the
 * next_row of the ppg_link call that followed step t), in_use / terminated / truncated uint8 0 / 1 (what a bool tensor holds),
 * values float64 (PPG_F64) or float32 (PPG_F32, widened exactly), returns / advantages float64.  For t = n_steps-1 .. 0 and
 * every row r of env b, each line one IEEE float64 operation in this order, no fused multiply-add:
 *   has    = t + 1 < n_steps && in_use[t][r] && !terminated[t][r] && !truncated[t][r] && 0 <= next_row[t][r] < S
 *   g_succ = has ? G[t+1][next_row[t][r]] : 0.0          (likewise a_succ from A[t+1], v_succ from values[t+1])
 *   G[t][r] = in_use ? reward + g_succ * gamma : 0.0
 *   A[t][r] = in_use ? ((reward + v_succ * gamma) - values[t][r]) + a_succ * (gamma * lam) : 0.0
 * gamma * lam is formed once in double on the host.  The call touches no env state and no library-owned buffer, and writes
 * every element of the outputs it is given.  Cases:
 *   - returns or advantages may be NULL (not both); advantages need values, returns alone ignore them (values may be NULL);
 *   - absent terms are selected, never multiplied away: a NaN or any other word in a row not in use, or in a successor slot that
 *     is not taken, reaches no output; rows not in use get +0.0.  The add of 0.0 * gamma still happens where there is no
 *     successor (a reward of -0.0 gives +0.0);
 *   - a next_row outside [0, S) means "no successor" like -1: no value from a tensor is used as an index unchecked;
 *   - the last step has no successor at all: the horizon's end is treated like an episode's;
 *   - PPG_EINVAL (text in ppg_last_error): n_steps < 1, a NULL input, both outputs NULL, advantages without values, a
 *     values_dtype that is neither code, a handle whose S is not 64 * (2 .. 6); nothing is launched then.
 * Asynchronous on `stream`. */
#define PPG_F64 0
#define PPG_F32 1
int ppg_backward(ppg_handle *h, int32_t n_steps, const double *reward, const int16_t *next_row, const uint8_t *in_use,
                 const uint8_t *terminated, const uint8_t *truncated, const void *values, int32_t values_dtype, /* values may be NULL */
                 double gamma, double lam, double *returns, double *advantages, void *stream);

/* ---- returns and advantages straight into sample order -----------------------------------------------------------------
 * ppg_backward_samples is ppg_backward for a learner whose minibatch is indexed by the slots of ppg_record_obs: it READS the critic's
 * values per sample (values[s][k]) and WRITES advantages and returns per sample (advantage[s][k], returns[s][k], float32), and on
 * request the per-env moments that advantage normalisation needs -- in ONE launch (one wavefront per env; csrc/ppg_backward.h), with
 * no [n_steps,B,S] tensor of values, returns or advantages anywhere.  It is defined to equal: scatter the values into [n_steps,B,S]
 * with 0 elsewhere, ppg_backward, pick the stored rows, round once to float32.  reward, next_row, in_use, terminated, truncated are
 * ppg_backward's tensors, contiguous device [n_steps,B,S]; st->slot is the int32 [st->horizon,B,S] table ppg_record_obs filled, of which
 * the first n_steps steps are read; B, S and pred_capacity (cp) are the handle's; s = 0 predators, 1 prey.
 *   Rows     for every (t, b, r) with t < n_steps: s = r < cp ? 0 : 1, k = st->slot[t][b][r],
 *              stored = in_use[t][b][r] && 0 <= k && k < st->capacity[s]
 *            (k is read from memory: it is compared before it becomes an address, a word outside is never followed).
 *   Values   V[t][b][r] = stored && values[s] ? widen(values[s][k]) : 0.0 -- float64 as it is (PPG_F64) or float32 widened exactly
 *            (PPG_F32), one dtype for both species.  A selection, never a multiplication: values[s][k] of a slot no stored row
 *            refers to is not even read, so a NaN there reaches no output.  values[s] == NULL: V = 0 for every row of that species.
 *   G, A     exactly the recursion of ppg_backward over reward, next_row, the flags and that V, unchanged: the same `has`
 *            condition, one IEEE float64 operation per line in the same order, no fused multiply-add, gamma * lam formed once in
 *            double on the host, a next_row outside [0, S) means no successor, the last step (t = n_steps - 1) has no successor.
 *   Stores   if stored: advantage[s][k] = (float)A[t][b][r] and returns[s][k] = (float)G[t][b][r] -- ONE rounding to nearest even, at
 *            the store.  Rows in use that the store dropped (slot -1, or a slot word outside the capacity) still take part in the
 *            recursion with V = 0 -- their successors and predecessors see them exactly as after the scatter with 0 -- and nothing
 *            is stored for them.  No other element of any output is written: not the slots at or above the cursor, not the slots of
 *            steps >= n_steps.  If two rows carry the same valid k (a corrupt slot tensor) one of the two values lands there and no
 *            address leaves the tensors.
 *   Outputs  advantage[] and returns[] are pairs: both pointers NULL or both set, and not both pairs NULL.  With advantage[] NULL
 *            the values are not read at all (returns do not depend on V).
 *   stats    (optional, needs advantage[]) float64 [B,2,3]: per env b and species s {count, sum A, sum A * A} over the stored rows, A
 *            being the float64 value BEFORE its rounding, in a fixed order so that it can be checked bit for bit: lane l of the
 *            env's wavefront owns rows 64q + l (cp is a multiple of 64: the species is uniform per q) and keeps three float64
 *            accumulators per species, started at +0.0; for t = n_steps-1 .. 0 and q ascending, if stored:
 *              n = n + 1.0;  sum = sum + A;  p = A * A;  sq = sq + p          (each one operation)
 *            then for m in 1, 2, 4, 8, 16, 32: x = x + x_of_lane(l ^ m) for each of the three (commutative: every lane ends with the
 *            same bits), and lane 0 stores stats[b][s][0..3).  All B * 2 * 3 elements are written.  The sum over the envs is the
 *            caller's: one reduction over [B].
 *   Not read st->obs, sample, action and cursor (they may be NULL); st->horizon only bounds n_steps and sizes slot.
 * PPG_EINVAL (text in ppg_last_error beginning "ppg_backward_samples:", nothing is launched): n_steps < 1 or n_steps > st->horizon; a
 * NULL input tensor; st, tg or st->slot NULL; a capacity < 0 or above INT32_MAX; horizon * B * S above INT32_MAX; only one pointer of
 * an output pair set; both output pairs NULL; stats without advantage[]; a values_dtype that is neither code (checked only if a
 * values pointer is set); a handle whose S is not 64 * (2 .. 6).
 * No atomics anywhere in the call.  It touches no env state and no library-owned buffer.  Asynchronous on `stream`. */
typedef struct ppg_sample_targets {
    const void *values[2];    /* [st->capacity[s]] per-sample critic values, float32 (PPG_F32) or float64 (PPG_F64);
                                 NULL: V = 0 for every row of that species */
    float  *advantage[2];     /* [st->capacity[s]]; both NULL or both set */
    float  *returns[2];       /* [st->capacity[s]]; both NULL or both set; not both pairs NULL */
    double *stats;            /* [B,2,3] {count, sum A, sum A*A} per env and species, or NULL; needs advantage[] */
} ppg_sample_targets;
int ppg_backward_samples(ppg_handle *h, int32_t n_steps, const double *reward, const int16_t *next_row,
                         const uint8_t *in_use, const uint8_t *terminated, const uint8_t *truncated,
                         const ppg_obs_store *st, const ppg_sample_targets *tg, int32_t values_dtype,
                         double gamma, double lam, void *stream);

/* ---- PPO's clipped loss and its gradients over one minibatch -------------------------------------------------------------
 * ppg_ppo_loss is the last step of the learner's side: from the columns the calls above stored per sample slot k of ONE species
 * (action, logp, dist, advantage, value target) and a learner's fresh logits and values for a minibatch of M samples it writes the
 * gradients of
 *     L = mean over the valid samples of ( -surr + vf_coeff * vfc - ent_coeff * H + kl_coeff * KL )
 * (the loss of RLlib's PPOTorchLearner.compute_loss_for_module) with respect to the logits and the values, and per-chunk partial sums
 * from which the caller composes the loss scalar and its statistics.  Two launches of one-wave workgroups over chunks of
 * PPG_PPO_CHUNK = 1024 minibatch rows (csrc/ppg_ppo.h), G = ceil(M / 1024); lane l of workgroup g owns rows i = 1024 g + 64 j + l,
 * j = 0 .. 15 ascending.  No atomics, nothing read back, no library-owned buffer.  All tensors are contiguous device memory.
 *   Rows     k = index ? index[i] : i.  Row i is VALID when 0 <= k < capacity (compared before k becomes an address), then
 *            0 <= action[k] < A (compared, never used as an index unchecked) and logp[k] is finite.  Validity is a selection, not a
 *            multiplication: an invalid row is not counted, adds nothing to any sum, gets +0.0 in grad_logits[i][0..A) and in
 *            grad_values[i], and nothing else of it is read -- a NaN in its logits row or its other columns reaches no output.
 *            Among valid rows everything propagates by IEEE rules: a NaN or +inf logit is not masked.
 *   Launch 1 ppg_ppo_count: workgroup g counts its valid rows (1.0 each, the order below) and stores partial[g][0].
 *   Launch 2 ppg_ppo_rows: every workgroup adds partial[0..G)[0] in ascending g: n; w = n > 0 ? 1 / n : 0.  Then per valid row, in
 *            float64, every line one IEEE operation, no fused multiply-add, one rounding to float32 at each store
 *            (l = logits[i], o = dist[k], a = action[k], sums over the actions in ascending order):
 *              m = max l_c (a NaN is never the maximum)       d_c = l_c - m        e_c = d_c == -inf ? 0 : exp(d_c)
 *              s = sum e_c      ls = log(s)      lp_c = d_c - ls      p_c = e_c / s
 *              (likewise mo, do_c, eo_c, so, lso, lq_c, q_c from o, if dist is given)
 *              r  = exp(lp_a - (double)logp[k])
 *              Ad = adv_norm ? ((double)advantage[k] - adv_norm[0]) * adv_norm[1] : (double)advantage[k]
 *              rc = r < 1 - clip ? 1 - clip : r > 1 + clip ? 1 + clip : r          (1 - clip and 1 + clip formed once in double)
 *              s1 = Ad * r      s2 = Ad * rc      clipped = s2 < s1      surr = clipped ? s2 : s1      (a tie, and a NaN, is unclipped)
 *              H  = 0 - sum over c with d_c != -inf of p_c * lp_c            (a masked action's addend is skipped, never 0 * inf)
 *              KL = sum over c with q_c != 0 of q_c * (lq_c - lp_c)         (+inf where q_c > 0 and the new logit is -inf)
 *              e  = (double)values[i] - (double)value_target[k]      vf = e * e      over = vf > vf_clip      vfc = over ? vf_clip : vf
 *              c1 = clipped ? 0 : s1
 *              g_c = d_c == -inf ? +0.0
 *                    : w * ( (ent_coeff * (p_c * (lp_c + H)) - c1 * ((c == a ? 1 : 0) - p_c)) + kl_coeff * (p_c - q_c) )
 *                                                                            (the last term only if dist is given)
 *              grad_logits[i][c] = (float)g_c       grad_values[i] = (float)(w * (vf_coeff * (over ? 0 : e + e)))
 *            Without values the value lines are not computed and grad_values is not written; without dist the KL lines are not.
 *   partial  float64 [G,8]: per workgroup g {n, sum surr, sum vfc, sum vf, sum H, sum KL, sum 1[clipped], sum ((double)logp[k] - lp_a)}
 *            over its valid rows; columns 2, 3 are +0.0 without values, column 5 without dist.  Each lane keeps its accumulators from
 *            +0.0 and adds its rows in ascending j; then for m in 1, 2, 4, 8, 16, 32: x = x + x_of_lane(l ^ m) (the order of
 *            ppg_backward_samples' stats) and lane 0 stores.  Column 0 is written only by launch 1 and columns 1..7 only by launch 2,
 *            so all G * 8 elements are written and `partial` needs no initial value.  The sum over g and the loss scalar are the
 *            caller's: one reduction over [G].
 *   Written  grad_logits [M,A] and grad_values [M] (if given) completely, partial completely; no input is written.
 * PPG_EINVAL (text in ppg_last_error beginning "ppg_ppo_loss:", nothing is launched): mb NULL; logits, action, logp, advantage,
 * grad_logits or partial NULL; M < 1 or above INT32_MAX; A outside 1..32; capacity < 0 or above INT32_MAX; only one of values /
 * value_target set; grad_values without values; kl_coeff != 0 without dist; clip or vf_clip negative or not finite.
 * The handle supplies the device, the stream ordering and the error text only: no env state is touched.  Asynchronous on `stream`. */
#define PPG_PPO_CHUNK 1024
typedef struct ppg_ppo_batch {
    int64_t M;                  /* minibatch rows, 1 .. INT32_MAX */
    int64_t capacity;           /* slots of the store columns, 0 .. INT32_MAX */
    int32_t A;                  /* actions, 1 .. 32 */
    int32_t reserved_;
    const int32_t *index;       /* [M] slot of minibatch row i, or NULL: k = i */
    const float *logits;        /* [M,A] the learner's new logits */
    const float *values;        /* [M] the critic's new values, or NULL: no value term (value_target must be NULL too) */
    const int8_t *action;       /* [capacity] */
    const float *logp;          /* [capacity] */
    const float *dist;          /* [capacity,A] the behaviour policy's logits, or NULL (kl_coeff must be 0) */
    const float *advantage;     /* [capacity] */
    const float *value_target;  /* [capacity] or NULL */
    const double *adv_norm;     /* DEVICE float64 [2] {shift, scale}, or NULL: the advantage as it is */
    double clip, vf_clip, vf_coeff, ent_coeff, kl_coeff;
} ppg_ppo_batch;
int ppg_ppo_loss(ppg_handle *h, const ppg_ppo_batch *mb, float *grad_logits, float *grad_values, double *partial, void *stream);

/* ---- policy inference next to the env (base_environment/tune_ppo_base_environment.py:106-141) ----------
 * The reference trains two PPO policies (predator_policy / prey_policy) with RLlib's DefaultPPOTorchRLModule and
 * model_config {conv_filters [[16,[3,3],1],[32,[3,3],1],[64,[3,3],1]], fcnet_hiddens [256,256], fcnet_activation relu}.
 * WHAT RLLIB BUILDS FROM THAT (pinned by the checkpoint the reference tree holds, .../shared_prey/experiments/PPO_v_APPO/.../
 * checkpoint_000099/learner_group/learner/rl_module/type_1_predator/module_state.pkl, ray 2.52.1; tests/golden/rllib_checkpoint/):
 * a 3-D Box is read channels-LAST -- the (C,R,R) observation is an image of C rows x R columns with R channels -- by a CNN encoder
 * of one ZeroPad2d + Conv2d(3x3, stride 1) + ReLU per conv_filters entry (keys encoder.actor_encoder.net.0.cnn.{1,4,7,...}),
 * whose output is permuted back to channels-last and flattened ([row][column][channel]); `fcnet_hiddens` is IGNORED for image
 * observations and the policy head is ONE Linear(flat -> n_actions) (pi.net.mlp.0) unless `head_fcnet_hiddens` is set.
 * ppg_policy_create_spec takes that network (and its variations: 1-6 convolutions, 0-2 hidden head layers, either image
 * reading, either flatten order); ppg_policy_act evaluates it for EVERY row in use of the handles' last call, reading the
 * observation rows in place (obs_pred / obs_prey of ppg_buffers) and writing the chosen action into actions[b][slot] -- the
 * observations never leave the GPU and what a consumer has to move per agent is one byte.  Arithmetic: bf16 operands, fp32
 * accumulation, on the matrix cores (v_mfma_f32_32x32x16_bf16 / 16x16x32); activations are rounded to bf16 between layers.
 * RLlib itself is not importable here: parity is pinned against a float32 PyTorch module with RLlib's parameter names and
 * shapes (predpreygrass_amd.policy.PolicyNet, loaded strictly from the real checkpoint) within the tolerance the tests state. */
typedef struct ppg_policy_weights {   /* HOST pointers, float32, PyTorch layouts */
    const float *conv_w[3];  /* Conv2d.weight [cout][cin][3][3]: cin = C / 16 / 32, cout = 16 / 32 / 64 */
    const float *conv_b[3];  /* Conv2d.bias [cout] */
    const float *fc_w[3];    /* Linear.weight [out][in]: [256][64*P] (input flattened channel-major), [256][256], [n_actions][256] */
    const float *fc_b[3];    /* Linear.bias [out] */
} ppg_policy_weights;

/* How the network reads the (4,R,R) observation as an image with C channels and P positions:
 *   PPG_POLICY_LAYOUT_CHW  channel-first: an R x R image with C = 4 channels (P = R*R) -- conv1 weight [16][4][3][3];
 *   PPG_POLICY_LAYOUT_HWC  channels-last: a 4 x R image with C = R channels (P = 4*R) -- conv1 weight [16][R][3][3].  This is how
 *                          RLlib's CNN encoder reads a 3-D Box (its observation spaces are [H, W, C]), i.e. what a module trained by
 *                          tune_ppo_base_environment.py:106-141 on Box(0, 100, (4,R,R)) holds.
 * The conv1 weight shape of a checkpoint tells the two apart (predpreygrass_amd.policy.load_rllib_state_dict). */
#define PPG_POLICY_LAYOUT_CHW 0
#define PPG_POLICY_LAYOUT_HWC 1

typedef struct ppg_policy ppg_policy;

#define PPG_POLICY_ARGMAX 0x0u  /* action = argmax of the logits (first maximum) */
#define PPG_POLICY_SAMPLE 0x1u  /* action ~ softmax(logits): Gumbel-max with Philox4x32-10 keyed by (seed, env, row) */
#define PPG_POLICY_SEED_ON_DEVICE 0x2u /* `seed` is the address of a uint64 in DEVICE memory that the kernel reads when it runs: a step
                                        * captured into a hipGraph (policy + ppg_step + an increment of that word) can then be replayed
                                        * with a fresh key every time.  Pipeline networks (the reference's) with both policies given. */

/* How the convolution output [channel][position] is flattened into the first Linear layer's input:
 *   PPG_POLICY_FLATTEN_NCHW  torch.flatten of a channel-first tensor: feature = channel * P + position
 *   PPG_POLICY_FLATTEN_NHWC  RLlib: TorchCNN permutes its output back to channels-last before nn.Flatten: feature = position * C + channel */
#define PPG_POLICY_FLATTEN_NCHW 0
#define PPG_POLICY_FLATTEN_NHWC 1
#define PPG_POLICY_MAX_CONV 6
#define PPG_POLICY_MAX_FC 3

typedef struct ppg_policy_spec {   /* weights: HOST pointers, float32, PyTorch layouts */
    int32_t obs_channels;   /* C of the (C,R,R) observation rows: 4; 5 with the walls variant's visibility channel; <= 8 */
    int32_t obs_range;      /* R <= 15 */
    int32_t n_actions;      /* <= 32 */
    int32_t layout;         /* PPG_POLICY_LAYOUT_* */
    int32_t flatten;        /* PPG_POLICY_FLATTEN_* */
    int32_t n_conv;         /* 1..PPG_POLICY_MAX_CONV convolutions 3x3, stride 1, "same" zero padding, ReLU */
    int32_t conv_out[PPG_POLICY_MAX_CONV];   /* output channels per layer: <= 16, <= 32, then <= 64 (multiples of 8) */
    int32_t n_fc;           /* 1..PPG_POLICY_MAX_FC Linear layers behind the flatten; the last one gives the logits, the others ReLU */
    int32_t fc_out[PPG_POLICY_MAX_FC];       /* hidden widths (<= 256), then n_actions */
    const float *conv_w[PPG_POLICY_MAX_CONV];  /* Conv2d.weight [cout][cin][3][3] */
    const float *conv_b[PPG_POLICY_MAX_CONV];  /* Conv2d.bias [cout] */
    const float *fc_w[PPG_POLICY_MAX_FC];      /* Linear.weight [out][in] */
    const float *fc_b[PPG_POLICY_MAX_FC];      /* Linear.bias [out] */
} ppg_policy_spec;

/* The general form.  n_fc == 1 (what RLlib builds: no hidden head layer) runs entirely in LDS -- one persistent launch per species
 * whose workgroups take the convolutions and the head of a few samples at a time; n_fc >= 2 needs n_conv == 3 with 16/32/64 channels
 * (the hidden layers are zero-padded to 256 features).  PPG_EINVAL with a message names anything else. */
int ppg_policy_create_spec(int32_t device, const ppg_policy_spec *spec, ppg_policy **out);
/* obs_range: the R of the species' (4,R,R) observations; n_actions <= 32.  The weights are repacked into MFMA fragment
 * order (bf16) on the device; the host arrays may be freed afterwards.  These two are ppg_policy_create_spec with 4 channels, three
 * convolutions 16/32/64, two hidden layers of 256 and the NCHW flatten (rounds 2-3's network; kept for its callers). */
int ppg_policy_create(int32_t device, int32_t obs_range, int32_t n_actions, const ppg_policy_weights *w, ppg_policy **out);
int ppg_policy_create_layout(int32_t device, int32_t obs_range, int32_t n_actions, int32_t layout, const ppg_policy_weights *w,
                             ppg_policy **out);
int ppg_policy_destroy(ppg_policy *p);
/* One forward pass of `pred` over the predator rows in use and of `prey` over the prey rows in use of all n handles (either
 * may be NULL: that species keeps whatever actions[] holds).  actions[k]: device int8 [B_k, S] of handle k.
 * logits_pred / logits_prey: optional device float [rows in use over all envs][n_actions], env-major in row order (the
 * order of ppg_pack); NULL = not wanted.  seed: Philox key of PPG_POLICY_SAMPLE (use a fresh value per step).
 * Asynchronous on `stream`, which the caller has ordered behind the handles' last step. */
int ppg_policy_act(ppg_policy *pred, ppg_policy *prey, ppg_handle *const *handles, int32_t n, int8_t *const *actions,
                   uint32_t flags, uint64_t seed, float *logits_pred, float *logits_prey, void *stream);
/* multiply-accumulates one observation costs in this network (for FLOP accounting: 2 flops each) */
uint64_t ppg_policy_macs_per_observation(const ppg_policy *p);
const char *ppg_policy_last_error(const ppg_policy *p);
/* Which kernels ppg_policy_create_spec would pick for this network and how they lay out a CU's 160 KB of LDS -- computed without a
 * device and without the weights (the pointers of `spec` are not read); for tests and for sizing.  Fills up to n of:
 *   out[0] kernel family: 0 FC chain (hidden head layers), 1 one-role direct-head kernels, 2 the same for more than three
 *          convolutions, 3 the two-role pipeline (three convolutions, <= 16 actions)
 *   out[1] samples per sub-group   out[2] dynamic LDS bytes per workgroup   out[3] threads per workgroup
 *   family 3 only: out[4] samples a workgroup's table holds, out[5] bytes of a sample's region, out[6] 8-byte row chunks a thread
 *   fetches per sub-group (0: one load per channel), out[7] samples covered per chunk load, out[8..10] byte offsets of the
 *   partial-sum area, the row area and the images, out[11] bytes of the row area
 * Returns PPG_EINVAL for a spec ppg_policy_create_spec would reject on its shape.  (Diagnostic: with the environment variable
 * PPG_POLICY_PIPE=0 set when a policy is created, a network of family 3 gets the kernels of family 1 -- same logits, bit for bit.) */
int ppg_policy_describe(const ppg_policy_spec *spec, int32_t *out, int32_t n);
/* The weight fragments ppg_policy_create_spec uploads for one layer, in MFMA operand order, as bfloat16 bit patterns -- computed
 * without a device, so that the repacking (which lane holds which weight of which k-step) can be checked on the CPU against a plain
 * convolution before a kernel ever runs (tests/test_policy.py).  what: 0 .. n_conv - 1 = that convolution for
 * v_mfma_f32_32x32x16_bf16, [row tile][k-step][lane][8]; PPG_POLICY_PACK_CONV1X = the first convolution as the two-role pipeline
 * takes it (v_mfma_f32_16x16x32_bf16, [kernel row][lane][8]; up to nine input channels); PPG_POLICY_PACK_HEAD = the single Linear head
 * of a network without hidden head layers (v_mfma_f32_16x16x32_bf16, [action tile][k-step][lane][8]).  *n_words = words the layer
 * takes; out == NULL or capacity too small: only the size is reported (PPG_OK). */
#define PPG_POLICY_PACK_CONV1X 100
#define PPG_POLICY_PACK_HEAD 200
#define PPG_POLICY_PACK_SLOTS 300 /* not weights: the two-role pipeline's slot table, one word per slot of a sub-group = sample << 8 |
                                   * position (0xFFFF: empty) -- which position a lane of an MFMA tile computes; ordered so that a tile's
                                   * cells fall into all LDS bank groups (csrc/ppg_policy_host.h: ppg_slot_table) */
int ppg_policy_pack(const ppg_policy_spec *spec, int32_t what, uint16_t *out, uint64_t capacity, uint64_t *n_words);

/* New weights for a policy that exists, from the DEVICE: the learner-to-actor hand-over without the host.  The weight pointers of
 * `spec` are DEVICE pointers on p's device -- float32, contiguous, PyTorch layouts, e.g. the parameters an optimiser has just stepped
 * -- and its shape must be the one `p` was created with: a difference in obs_channels, obs_range, n_actions, layout, flatten, n_conv,
 * conv_out[], n_fc or fc_out[] is PPG_EINVAL with a message that names the field; so are a NULL p, a NULL spec and a NULL weight
 * pointer of a layer the shape has.  One kernel (csrc/ppg_policy.h: ppg_policy_repack) gathers the parameters through a repack map
 * into the fragment order and writes them INTO THE POLICY'S EXISTING WEIGHT IMAGE, to the bits ppg_policy_create_spec would have
 * uploaded for them: no address the policy kernels read changes, so a hipGraph captured around ppg_policy_act earlier acts with the new
 * weights at its next replay.  The FIRST update of a policy builds the map, allocates it on the device and uploads it -- that call may
 * block and must not stand inside a stream capture; the map is freed by ppg_policy_destroy.  Every LATER update only launches: no
 * allocation, no host wait, no copy; asynchronous on `stream` and legal inside a stream capture (the parameters are read when the
 * kernel RUNS, so a captured update picks up whatever they hold at each replay).
 * ORDER: an update is ordered like an act.  Put it on a stream behind the last ppg_policy_act that should see the old weights and in
 * front of the first that should see the new ones, and behind whatever wrote the parameters.  The two-species ppg_policy_act forks
 * its side stream from `stream` and joins back into it, so same-stream order is enough.
 * Non-finite parameters are carried as non-finite, with unspecified bit patterns. */
int ppg_policy_update(ppg_policy *p, const ppg_policy_spec *spec, void *stream);

/* The byte image of a network's weights as ppg_policy_create_spec uploads it -- computed without a device, like ppg_policy_pack, so that
 * ppg_policy_update's map can be checked on the CPU.  The image: eleven arrays one behind the other, each padded with zeros to a
 * multiple of 256 bytes -- the convolutions 0-5, three arrays of the linear layers (a network without hidden head layers: the head,
 * the head per wavefront, nothing), PPG_POLICY_PACK_CONV1X's, PPG_POLICY_PACK_SLOTS' (with the kernels PPG_POLICY_PIPE picks: see
 * ppg_policy_describe) -- then 560 floats of biases.  what:
 *   PPG_POLICY_IMAGE_PACKED    the image, from the host weights of `spec`
 *   PPG_POLICY_IMAGE_REPACKED  the same bytes made the update's way: a buffer filled with 0xA5 that holds nothing but the slot table's
 *                              array, then the map and the word function of ppg_policy_update run on the CPU over the host weights
 *   PPG_POLICY_IMAGE_MAP       the map itself, int32 words (the weight pointers of `spec` are not read): a header of 32 words --
 *                              [0] 32, [1] W = bf16 words covered = image bytes [0, 2 W), every array in front of the slot table,
 *                              [2] floats of the bias block, [3] bytes of the image, [4] byte offset of the bias block, [5 + l] byte
 *                              offset of array l, [16 + l] bf16 words of array l (l < 11) -- then W entries, one per bf16 word from
 *                              image byte 0 on, then one per float of the bias block.  An entry: 0 = the constant zero; otherwise
 *                              bits 24-28 = 1 + tensor (conv_w[0..5] 0-5, conv_b[0..5] 6-11, fc_w[0..2] 12-14, fc_b[0..2] 15-17), bits
 *                              0-23 = the element of that tensor, bit 29 set = not the element b itself but what bfloat16 leaves of
 *                              it, b - float(bf16(b)) (the second word of a convolution's bias).  Weight entries are rounded to
 *                              bfloat16 (to nearest even, in integer arithmetic), bias entries are copied.
 * *n_bytes = bytes of the result; out == NULL or capacity (bytes) too small: only the size is reported (PPG_OK). */
#define PPG_POLICY_IMAGE_PACKED 0
#define PPG_POLICY_IMAGE_REPACKED 1
#define PPG_POLICY_IMAGE_MAP 2
int ppg_policy_image(const ppg_policy_spec *spec, int32_t what, void *out, uint64_t capacity, uint64_t *n_bytes);

/* The network of a policy over a DENSE tensor of observation rows -- the sample store ppg_record_obs fills, or any [rows][C][R][R]
 * tensor -- instead of the rows in use of a handle: a critic's values for every stored sample (a critic is a network with
 * n_actions = 1: its one "logit" is the value), or the actor's logits under its current weights, on the matrix cores.  The forward
 * kernels are ppg_policy_act's, launched once for one species; what differs is where their plan comes from: a kernel of its own,
 * ppg_policy_plan_rows in csrc/ppg_policy.h, writes it in closed form from the row count (csrc/ppg_policy_plan.h).
 * Rows [0, min(max(count, 0), capacity)) of `out` receive the float32 outputs, BIT FOR BIT what ppg_policy_act writes into its logits
 * tensor for the same observation row and weights (same kernels, same arithmetic; a row's result does not depend on its position or
 * on the count).  Rows at and behind the count keep what they held.  Outputs are those of PPG_POLICY_ARGMAX: no Philox key is
 * involved, and the action byte the kernels store per sample goes to a scratch the policy owns.
 * The count is `count`, or -- count_dev != NULL -- one int64 in device memory that the plan kernel reads WHEN IT RUNS (a word of the
 * store's cursor): nothing is read back and the host never waits.
 * The policy keeps a plan buffer and the action scratch for this call, apart from ppg_policy_act's plan (an evaluate between two acts
 * moves nothing a graph captured around ppg_policy_act reads); they are allocated at the first call and whenever `capacity` exceeds
 * every earlier call's, and freed by ppg_policy_destroy.  Such a call must not stand inside a stream capture; every LATER call at a
 * capacity up to that one only launches (two kernels) and can be captured.
 * ORDER: the forward kernels' scratch belongs to the policy, so an evaluate is ordered like an act: on one stream with the policy's
 * other calls (act, update, evaluate), and behind whatever wrote the rows and the count.
 * PPG_EINVAL with a message, before anything is launched: p or rows NULL, obs or out NULL with capacity > 0, an obs_dtype other than
 * 0 / 1 / 2 (the cell layout is not taken), capacity < 0 or above 2^30.  capacity == 0, or count <= 0 with count_dev NULL: PPG_OK
 * without a launch.  The checks of ppg_policy_act that speak about a handle (nine actions in the base env, 64 predator rows) do not
 * apply: there is no handle. */
typedef struct ppg_policy_rows {
    const void *obs;          /* device, dense [capacity][C][R][R], element type obs_dtype */
    int32_t obs_dtype;        /* ppg_config.obs_dtype's codes: 0 float64, 1 float32, 2 bfloat16 (not the cell layout) */
    int64_t capacity;         /* rows the tensors have */
    int64_t count;            /* rows to evaluate, used when count_dev is NULL */
    const int64_t *count_dev; /* or: one int64 on the device, read by the plan kernel when it runs */
    float *out;               /* device, float32 [capacity][n_actions] */
} ppg_policy_rows;
int ppg_policy_evaluate(ppg_policy *p, const ppg_policy_rows *rows, void *stream);

/* Diagnostic, device-free like ppg_policy_image: the words the plan kernel of ppg_policy_evaluate writes for `count` of `capacity` rows
 * and a forward grid of `slots` workgroups, made by the same inline functions on the CPU -- so that the plan can be checked where
 * there is no GPU.  The words: [0] rows to evaluate, [1], [2] as the network's kernels read them (FC chain: full tiles of 128, samples
 * per tile of the last round; direct head / pipeline: samples of a workgroup's share, tiles per workgroup), then the exclusive prefix
 * sums of the ceil(capacity / PPG_POLICY_ROWS_CHUNK) pseudo-envs the rows are read as, then the pseudo-env of every tile's first
 * sample.  *n_words = their number; out == NULL or capacity_words too small: only the size is reported (PPG_OK).  PPG_EINVAL: a spec
 * ppg_policy_create_spec would reject on its shape, slots < 1, capacity outside [0, 2^30].  The weight pointers are not read. */
#define PPG_POLICY_ROWS_CHUNK 128   /* rows per pseudo-env; the results of ppg_policy_evaluate do not depend on it */
int ppg_policy_rows_plan(const ppg_policy_spec *spec, int32_t slots, int64_t capacity, int64_t count, uint32_t *out,
                         uint64_t capacity_words, uint64_t *n_words);

/* ---- the policy networks' training pass: minibatch forward and backward in float32 -----------------------------------------
 * ppg_net_forward and ppg_net_backward run a network of the shapes ppg_policy_create_spec accepts (anything else: PPG_EINVAL with
 * the same words) over a minibatch of M rows taken from a dense [capacity][C][R][R] observation tensor through an int32 slot index,
 * forwards (one launch) and backwards (two launches), in float32 throughout -- the learner's side of a PPO step, where ppg_policy_act
 * and ppg_policy_evaluate are the actor's (bf16 operands).  A critic is the same network with n_actions == 1.  csrc/ppg_net.h.
 *   Weights  the weight pointers of `spec` are DEVICE pointers, float32, contiguous, PyTorch layouts, exactly as ppg_policy_update takes
 *            them: the parameters where the optimiser keeps them, read when the kernels run.  No packed copy exists.
 *   Rows     k = index ? index[i] : i.  A row with 0 <= k < capacity (compared before k becomes an address) reads observation row k,
 *            float64 and bfloat16 converted to float32 as obs.to(torch.float32) does.  Any other row is a SELECTION: nothing of it is
 *            read (no observation, not its grad_out row), its out row is +0.0, and it adds nothing to any gradient.
 *   Tiles    a workgroup (256 threads) takes tiles of TS consecutive minibatch rows (TS = 4, 2 or 1: the largest with two buffers of
 *            TS x the widest layer in 80 KB of LDS, else 1).  Workgroups are persistent: G = groups ? min(groups, tiles) :
 *            min(tiles, 1024), workgroup g takes tiles g, g + G, ...
 *   Forward  every convolution (zero pad 1, 3x3, stride 1, bias, ReLU) and every linear layer (ReLU on all but the last) with the
 *            tile's activations in LDS; out[M][n_actions] float32; every post-ReLU activation goes to `workspace`, which the
 *            backward call of the same batch reads.  A chain starts from the bias (convolutions) or from +0.0 with the bias added
 *            last (linear layers), products enter by fmaf.
 *   Backward launch 1, per tile, from grad_out[M][n_actions]: the ReLU mask is activation > 0; per layer the tile's contribution to
 *            every weight and bias gradient (one fmaf chain over the tile's rows ascending, then positions ascending) is stored
 *            (first tile of the workgroup) or added (later tiles, ascending) into partial[g][n_params].  Launch 2 adds the G rows in
 *            ascending g and writes the gradients through the pointers of `grads` (a ppg_policy_spec of which only the weight
 *            pointers are read: Conv2d.weight [cout][cin][3][3], Linear.weight [out][in], the biases).  No atomics: for a given M
 *            and G the gradients are the same bits from run to run.  `partial` needs no initial value.
 *   Order    of the parameters in partial's rows (and in a flat gradient buffer a caller lays its `grads` pointers over):
 *            conv0.weight, conv0.bias, conv1.weight, ..., fc0.weight, fc0.bias, ...
 * ppg_net_bytes needs no device and does not read the weight pointers: out[0] = bytes of the workspace for M rows, out[1] = bytes
 * of partial (G rows), out[2] = n_params, out[3] = TS.  PPG_EINVAL: spec or out NULL, a network outside the set, M outside
 * [1, 2^24], groups < 0 (the text: ppg_last_error(NULL)).
 * PPG_EINVAL (text in ppg_last_error beginning "ppg_net_forward:" / "ppg_net_backward:", nothing is launched, nothing written): spec or
 * mb NULL; obs (with capacity > 0), out (forward) or workspace NULL; grad_out, grads or partial NULL; a NULL weight (gradient) pointer of a
 * layer the shape has; M outside [1, 2^24]; capacity outside [0, INT32_MAX]; groups < 0; an obs_dtype other than 0 / 1 / 2;
 * workspace_bytes / partial_bytes smaller than ppg_net_bytes says; a network outside the set.
 * The handle supplies the device, the stream ordering and the error text only.  All three calls are asynchronous on `stream`,
 * allocate nothing and can be captured in a graph (a network whose tile needs more than 64 KB of LDS -- ppg_net_bytes' TS x the widest layer x 8
 * bytes -- has the kernel's limit raised by a host call at its FIRST launch on a device: run that launch uncaptured once).  `mb` of ppg_net_backward must be the batch of the forward call that filled
 * the workspace. */
typedef struct ppg_net_batch {
    const void *obs;          /* device, dense [capacity][C][R][R], element type obs_dtype */
    int32_t obs_dtype;        /* 0 float64, 1 float32, 2 bfloat16 */
    int32_t groups;           /* 0: automatic; otherwise the number of workgroups G (at most the number of tiles, at most 1024) */
    int64_t capacity;         /* rows of obs, 0 .. INT32_MAX */
    const int32_t *index;     /* [M] slot of minibatch row i, or NULL: k = i */
    int64_t M;                /* minibatch rows, 1 .. 2^24 */
    float *out;               /* [M][n_actions]; not looked at by ppg_net_backward */
    float *workspace;         /* the activations, workspace_bytes >= ppg_net_bytes' out[0] */
    uint64_t workspace_bytes;
} ppg_net_batch;
int ppg_net_bytes(const ppg_policy_spec *spec, int64_t M, int32_t groups, uint64_t out[4]);
int ppg_net_forward(ppg_handle *h, const ppg_policy_spec *spec, const ppg_net_batch *mb, void *stream);
int ppg_net_backward(ppg_handle *h, const ppg_policy_spec *spec, const ppg_net_batch *mb, const float *grad_out,
                     const ppg_policy_spec *grads, float *partial, uint64_t partial_bytes, void *stream);

/* A device buffer for the caller-owned observation tensors whose physical pages are picked at random from a stretch of device
 * memory `spread` times its size (HIP virtual memory management: spread x as many 2 MB chunks are created, a random subset is
 * mapped in random order, the rest is given back at once).  Optional -- any device pointer works as obs_pred / obs_prey -- but where
 * the pages of those two tensors lie decides how fast HBM takes the step's scattered 1 KB pieces: 62-64 us per 4096-env step with
 * spread 32-64 against 62-91 us for what hipMalloc happens to return and 105-121 us for physically contiguous memory (profiles/EXPERIMENTS.md,
 * round 3).  Costs: spread 32 at 1.8 GB takes about 2.5 s and 58 GB of transient device memory; if the device cannot hold the
 * pool the spread shrinks, and the transient pool never takes more than half of the memory that is free when it is built.  Not in the
 * CPU test build.  ppg_free_spread gives the physical memory back and RETIRES the virtual range
 * (a re-used range was seen to go through stale translations).  Returns PPG_OK or an error code (ppg_spread_last_error()). */
int ppg_alloc_spread(int32_t device, uint64_t bytes, int32_t spread, uint64_t seed, void **out);
int ppg_free_spread(void *ptr);
/* what this process holds / has given up: bytes mapped now, and the virtual ranges (count, bytes) ppg_free_spread has retired.  Any
 * pointer may be NULL. */
int ppg_spread_stats(uint64_t *live_bytes, uint64_t *retired_ranges, uint64_t *retired_bytes);
const char *ppg_spread_last_error(void);   /* of the calling thread */

/* Sort key of the decimal string of `id` (digits d: sum (d+1)*11^(5-pos)); host helper. */
uint32_t ppg_lexkey(uint32_t id);

/* Name of the kernel ppg_step launches for this handle right now (it depends on the variant, the row capacity and -- through
 * ppg_set_envs_in_flight -- on how full the GPU is: one, two, four or eight wavefronts per env).  Diagnostic: profiles name it. */
const char *ppg_step_kernel_name(ppg_handle *h);

/* Dynamic LDS bytes per wavefront the step kernel uses for this handle (diagnostic). */
int32_t ppg_lds_bytes(const ppg_handle *h);

const char *ppg_last_error(const ppg_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* PPG_H */
