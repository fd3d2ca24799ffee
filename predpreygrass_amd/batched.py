"""BatchedPredPreyGrass: B independent PredPreyGrass grids stepped in lockstep on one MI355X.

Host code is plumbing only: it owns the PyTorch-ROCm tensors (state, actions, observations),
hands their raw pointers to libppg_hip.so through the C ABI of include/ppg.h and launches one
HIP kernel per call on torch's current stream.  All environment logic
(predpreygrass_rllib_env.py:219-473 of the reference) runs in predpreygrass_amd/csrc/ppg_kernel.h.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch

from . import _abi
from .config import resolve_config

PREDATOR, PREY = 0, 1
PRED_CAPACITY = 64                # predator rows per env by default
PRED_CAPACITIES = (64, 128)       # 128: one-wave kernels only -- base family (no drive channels) and second generation without walls,
                                  # prey_capacity 128 or 256; no policy kernels (include/ppg.h: ppg_config.pred_capacity)


def lexkey(ids) -> np.ndarray:
    """Sort key of the decimal id strings: same order as list.sort() on "prey_<id>"
    (predpreygrass_rllib_env.py:468); mirrors ppg_lexkey() in include/ppg.h."""
    ids = np.asarray(ids, dtype=np.int64)
    out = np.zeros(ids.shape, dtype=np.int64)
    flat, o = ids.reshape(-1), out.reshape(-1)
    for n, v in enumerate(flat):
        s = str(int(v))
        o[n] = sum((ord(ch) - 48 + 1) * 11 ** (5 - i) for i, ch in enumerate(s))
    return out.astype(np.int32)


def agent_name(type_: int, id_: int) -> str:
    return ("predator_%d" if type_ == PREDATOR else "prey_%d") % int(id_)


def _alloc_on(device, stream, fn):
    """fn() -- an allocation, with its fill if it has one -- for a launch on `stream`.  A torch.cuda.Stream: under
    `torch.cuda.stream(stream)`, so the fill runs on that stream and the caching allocator knows which stream uses the blocks.  A raw
    hipStream_t handle is unknown to torch: on the current stream, which the host then waits for -- the fill has to be complete, and a
    recycled block no longer in use there, before the launch runs.  No stream, or the CPU (emulated library): plainly."""
    if device.type != "cuda" or stream is None:
        return fn()
    if hasattr(stream, "cuda_stream"):
        with torch.cuda.stream(stream):
            return fn()
    out = fn()
    torch.cuda.current_stream(device).synchronize()
    return out


def capture_graph(device, body):
    """body() captured into a torch.cuda.CUDAGraph, after one uncaptured pass on a fresh side stream ordered behind the current stream
    (lazy allocations and attribute calls of the library and of the env must not fall into the capture); the current stream waits for
    that pass and the device is synchronised before the capture starts."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    return graph


def _ptr(x):
    """The address of a tensor as a launch argument; None stays None."""
    return None if x is None else C.c_void_p(x.data_ptr())


def net_grad_offsets(net):
    """Element offsets of a `policy.PolicyNet`'s parameters in the flat gradient buffer of net_backward(): conv0.weight, conv0.bias, ...,
    fc0.weight, fc0.bias, ... (include/ppg.h), and behind them the total."""
    offsets = [0]
    for m in net.conv + net.fc:
        for p in (m.weight, m.bias):
            offsets.append(offsets[-1] + p.numel())
    return offsets


def net_grad_views(net, flat):
    """[(parameter, view of `flat` of its shape)] in the order of net_grad_offsets()."""
    offsets = net_grad_offsets(net)
    params = [p for m in net.conv + net.fc for p in (m.weight, m.bias)]
    return [(p, flat[o:o + p.numel()].view(p.shape)) for p, o in zip(params, offsets)]


class BatchedPredPreyGrass:
    """Tensor API.

    Rows: ``[0, pred_capacity)`` predators (``pred_capacity`` 64, or 128 with ``prey_capacity`` 128 or 256 and
    one wave per env), ``[pred_capacity, pred_capacity + prey_capacity)`` prey.  Within a type the rows of
    the last call are ordered like the dict the reference's ``step()`` returns:
    survivors (incl. agents that died in that call) followed by newborns.  ``actions[b, row]``
    answers the observation in the same row of the previous call; rows that are dead, unused or
    deliberately left out of the action dict hold ``ACTION_NONE`` (-1).
    """

    def __init__(self, config=None, batch_size=1, device=None, obs_dtype=torch.float64,
                 prey_capacity=128, seed=0, _library=None, obs_spread=0, pred_capacity=PRED_CAPACITY):
        """obs_spread = N > 1: the two observation tensors live in memory from `ppg_alloc_spread` (include/ppg.h) -- physical pages
        picked at random from a stretch of device memory N times their size, which is what HBM wants for the step's scattered writes
        (profiles/EXPERIMENTS.md, round 3; N = 32 costs a few seconds and N x the tensors' size of transient device memory).  They stay valid
        until close()."""
        cfg = resolve_config(config)
        self._init_common(cfg, batch_size, device, obs_dtype, _library, obs_spread)
        self.P0, self.Q0 = int(cfg["n_initial_active_predator"]), int(cfg["n_initial_active_prey"])
        # drive-conditioned variant (drive_conditioned_environment/predpreygrass_rllib_env.py:54-89): extra observation
        # channels filled with per-agent scalars; absent / False = the base environment
        drive = bool(cfg.get("enable_drive_channels", False))
        drive_lists = (list(cfg.get("predator_drive_channels", _abi.DEFAULT_PREDATOR_DRIVES)) if drive else [],
                       list(cfg.get("prey_drive_channels", _abi.DEFAULT_PREY_DRIVES)) if drive else [])
        for lst in drive_lists:
            for name in lst:
                if name not in _abi.DRIVE_KINDS:
                    raise ValueError(f"Unknown drive feature: {name!r}")   # its :610
            if len(lst) > 4:
                raise ValueError("at most 4 drive channels per species")
        self.obs_channels_pred, self.obs_channels_prey = 4 + len(drive_lists[0]), 4 + len(drive_lists[1])
        self._alloc_buffers(prey_capacity, pred_capacity)
        NG = self.grass_capacity

        c = _abi.PpgConfig()
        for t in range(2):
            c.n_drive[t] = len(drive_lists[t])
            for k, name in enumerate(drive_lists[t]):
                c.drive_kind[t][k] = _abi.DRIVE_KINDS[name]
        c.hunger_safe_energy[0] = float(cfg.get("predator_hunger_safe_energy", cfg["initial_energy_predator"]))
        c.hunger_safe_energy[1] = float(cfg.get("prey_hunger_safe_energy", cfg["initial_energy_prey"]))
        c.prey_opportunity_normalizer = float(cfg.get("prey_opportunity_normalizer", cfg["initial_energy_prey"] * 3))
        c.predator_danger_normalizer = float(cfg.get("predator_danger_normalizer", cfg["initial_energy_predator"] * 2))
        c.grass_opportunity_normalizer = float(cfg.get("grass_opportunity_normalizer", cfg["initial_energy_grass"] * 5))
        c.abi_version = _abi.ABI_VERSION
        c.grid_size, c.predator_obs_range, c.prey_obs_range = self.grid_size, self.Rp, self.Rq
        c.max_steps = int(cfg["max_steps"])
        c.n_possible_predators, c.n_possible_prey = int(cfg["n_possible_predators"]), int(cfg["n_possible_prey"])
        c.n_initial_predators, c.n_initial_prey, c.n_grass = self.P0, self.Q0, self.n_grass
        c.pred_capacity, c.prey_capacity, c.grass_capacity = self.pred_capacity, self.prey_capacity, NG
        c.obs_dtype = self._abi_obs_dtype()
        for k_cfg, k_abi in [
            ("reward_predator_catch_prey",) * 2, ("reward_prey_eat_grass",) * 2, ("reward_predator_step",) * 2,
            ("reward_prey_step",) * 2, ("penalty_prey_caught",) * 2, ("reproduction_reward_predator",) * 2,
            ("reproduction_reward_prey",) * 2, ("energy_loss_per_step_predator",) * 2,
            ("energy_loss_per_step_prey",) * 2, ("predator_creation_energy_threshold",) * 2,
            ("prey_creation_energy_threshold",) * 2, ("initial_energy_predator",) * 2,
            ("initial_energy_prey",) * 2, ("initial_energy_grass",) * 2, ("energy_gain_per_step_grass",) * 2,
        ]:
            setattr(c, k_abi, float(cfg[k_cfg]))
        # seasonal variant keys (base_environment_seasonal/config_env.py:35-40); absent -> base environment
        c.season_length_steps = int(cfg.get("season_length_steps", 0) or 0)
        c.season_high_multiplier = float(cfg.get("season_high_multiplier", 1.0))
        c.season_low_multiplier = float(cfg.get("season_low_multiplier", 1.0))
        modes = {"sparse": 0, "dense_energy_delta": 1, "dense_energy_delta_plus_reproduction": 2}
        if cfg.get("reward_mode", "sparse") not in modes:
            raise ValueError(f"reward_mode must be one of {sorted(modes)}")
        c.reward_mode = modes[cfg.get("reward_mode", "sparse")]
        # kickback variant keys (project_reward_shaping/base_environment_sparse_rewards_plus_kickback/config_env.py:24-25)
        c.kickback = int("kickback_reward_predator" in cfg or "kickback_reward_prey" in cfg)
        c.kickback_reward_predator = float(cfg.get("kickback_reward_predator", 10.0))
        c.kickback_reward_prey = float(cfg.get("kickback_reward_prey", 10.0))
        if c.kickback and c.reward_mode != 0:
            raise ValueError("the kickback rewards are defined on top of the sparse reward mode only")
        self._create_handle(c, self._lib.ppg_create)
        self.set_seeds(seed)

    # ------------------------------------------------------------------
    def _init_common(self, cfg, batch_size, device, obs_dtype, _library, obs_spread):
        """What every family's __init__ starts with: the config, the library and its device, the geometry the buffers are sized from."""
        self.config = cfg
        self._obs_spread = int(obs_spread)
        self.batch_size = int(batch_size)
        self._emulated = _library is not None
        self._link_rows = None   # (prev_row, next_row) of link(), allocated on first use
        if _library is None:
            # the product path: HIP on a real GPU, or an exception
            self._lib = _abi.load_hip_library()
            if not torch.cuda.is_available():
                raise RuntimeError("predpreygrass_amd needs a ROCm GPU (gfx950); torch.cuda.is_available() is False")
            self.device = torch.device(device if device is not None else "cuda:0")
            if self.device.type != "cuda":
                raise RuntimeError(f"device must be a cuda (ROCm) device, got {self.device}")
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
        else:
            # test hook (tests/wave_emu): the same kernel source compiled for the CPU wave emulator
            self._lib = _library
            self.device = torch.device("cpu")
        # float64 = the reference's observations bit for bit; float32; bfloat16 = compact rows for a policy that runs next to the env
        # (FusedPolicy stages them without conversion: its logits are bit-identical to those from the float64 rows)
        if obs_dtype not in (torch.float64, torch.float32, torch.bfloat16):
            raise ValueError("obs_dtype must be torch.float64, torch.float32 or torch.bfloat16")
        self.obs_dtype = obs_dtype
        self.grid_size = int(cfg["grid_size"])
        self.Rp, self.Rq = int(cfg["predator_obs_range"]), int(cfg["prey_obs_range"])
        self.n_grass = int(cfg["initial_num_grass"])

    def _abi_obs_dtype(self):
        return {torch.float64: 0, torch.float32: 1, torch.bfloat16: 2}[self.obs_dtype]

    def _alloc_buffers(self, prey_capacity, pred_capacity=PRED_CAPACITY):
        if pred_capacity not in PRED_CAPACITIES:
            raise ValueError(f"pred_capacity must be one of {PRED_CAPACITIES}, got {pred_capacity!r}")
        self.pred_capacity = int(pred_capacity)
        self.prey_capacity = int(prey_capacity)
        if self.n_grass > 255 and self.prey_capacity < 256:
            self.prey_capacity = 256   # up to 128 prey rows the kernels use 8-bit cell maps: at most 255 grass patches
        self.S = self.pred_capacity + self.prey_capacity
        self.grass_capacity = max(64, (self.n_grass + 63) // 64 * 64)
        B, S, NG, dev = self.batch_size, self.S, self.grass_capacity, self.device

        def z(shape, dtype):
            return torch.zeros(shape, dtype=dtype, device=dev)

        self.row_xy = z((B, S), torch.int16)
        self.row_energy = z((B, S), torch.float64)
        self.row_id = z((B, S), torch.int32)
        self.row_key = z((B, S), torch.int32)
        self.row_cumrew = z((B, S), torch.float64)
        self.row_flags = z((B, S), torch.uint8)
        self.row_reward = z((B, S), torch.float64)
        self.row_parent = torch.full((B, S), -1, dtype=torch.int32, device=dev)
        self.row_lastrep = z((B, S), torch.int32)  # second generation only (agent_last_reproduction)
        self.wall_bits = z((B, (self.grid_size * self.grid_size + 31) // 32), torch.int32)  # walls variant only
        self.row_info = z((B, S), torch.uint8)                                               # walls variant only
        self.env_state = z((B, _abi.ENV_WORDS), torch.int32)
        self.env_seed = z((B,), torch.int64)
        self.grass_xy = z((B, NG), torch.int16)
        self.grass_energy = z((B, NG), torch.float64)
        self.obs_pred = self._obs_tensor((B, self.pred_capacity, self.obs_channels_pred, self.Rp, self.Rp), seed_salt=1)
        self.obs_prey = self._obs_tensor((B, self.prey_capacity, self.obs_channels_prey, self.Rq, self.Rq), seed_salt=2)
        self.actions = torch.full((B, S), _abi.ACTION_NONE, dtype=torch.int8, device=dev)
        self._row_index = torch.arange(S, device=dev, dtype=torch.int32).unsqueeze(0)   # (live_mask()'s row numbers)

    def _obs_tensor(self, shape, seed_salt=0):
        """An observation tensor: from torch's allocator, or (obs_spread > 1, HIP library) on spread physical pages."""
        spread = getattr(self, "_obs_spread", 0)
        if spread <= 1 or self.device.type != "cuda" or not hasattr(self._lib, "ppg_alloc_spread"):
            return torch.zeros(shape, dtype=self.obs_dtype, device=self.device)
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=self.obs_dtype).element_size()
        ptr = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        rc = self._lib.ppg_alloc_spread(dev_index, nbytes, spread, (id(self) << 4) ^ seed_salt, C.byref(ptr))
        if rc != 0:
            raise RuntimeError(f"ppg_alloc_spread failed ({rc}): {self._lib.ppg_spread_last_error().decode()}")

        class _Holder:   # what torch.as_tensor needs to see device memory it does not own
            pass

        holder = _Holder()
        holder.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr.value, False), "version": 2}
        # THE MAPPING LIVES AS LONG AS THE MEMORY IS REFERENCED: torch keeps `holder` alive until the last tensor (or view, or
        # tensor returned by reset_batch / step_batch) over this storage is gone, and only then are the pages unmapped -- never in
        # close(), which a caller may well outlive with an observation tensor in hand (touching unmapped memory is a GPU fault)
        weakref.finalize(holder, self._lib.ppg_free_spread, C.c_void_p(ptr.value))
        with torch.cuda.device(self.device):
            t = torch.as_tensor(holder, device=self.device).view(self.obs_dtype).view(shape)
            t.zero_()
        return t

    def _create_handle(self, c, create_fn):
        bufs = _abi.PpgBuffers()
        for name in _abi._BUF_FIELDS:
            setattr(bufs, name, getattr(self, name).data_ptr())
        self._handle = C.c_void_p()
        dev_index = self.device.index if self.device.type == "cuda" else 0
        rc = create_fn(C.byref(c), self.batch_size, dev_index, C.byref(bufs), C.byref(self._handle))
        if rc != 0:
            self._handle = None   # (the message is then the library's, not a handle's)
        self._check(rc, "ppg_create", value_error=True)  # e.g. "Cannot place more unique positions than grid cells."
        self.lds_bytes = int(self._lib.ppg_lds_bytes(self._handle))

    # ------------------------------------------------------------------
    def close(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            self._lib.ppg_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, stream=None):
        """hipStream_t for a launch: an explicit torch.cuda.Stream / raw handle, else torch's current stream."""
        if self.device.type != "cuda":
            return None
        if stream is None:
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))

    def _check(self, rc, what, value_error=False):
        """Raise unless rc is 0.  value_error: -1 is the library's refusal of an argument and raises ValueError with its message alone."""
        if rc != 0:
            msg = self._lib.ppg_last_error(self._handle).decode()
            if value_error and rc == -1:
                raise ValueError(msg)
            raise RuntimeError(f"{what} failed ({rc}): {msg}")

    def _tensor_arg(self, name, x, dtypes, shape):
        """The pointer of a tensor argument of a launch; ValueError unless it is a contiguous tensor of one of `dtypes` and of `shape`
        (None = any size in that dimension) on the env's device."""
        got = tuple(x.shape)
        if x.dtype not in dtypes or (got != shape and (len(got) != len(shape) or any(n not in (None, g) for n, g in zip(shape, got)))) \
                or x.device != self.device or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {' / '.join(str(d) for d in dtypes)} tensor "
                             f"[{','.join('*' if n is None else str(n) for n in shape)}] on {self.device}, not a"
                             f"{'' if x.is_contiguous() else ' non-contiguous'} {x.dtype} tensor {list(got)} on {x.device}")
        return C.c_void_p(x.data_ptr())

    def _step_args(self, actions, random_actions, auto_reset, act_rank=None, n_steps=None):
        """(flags, actions pointer, rank pointer) of a step launch.  n_steps: of a rollout, whose action tape is [n_steps,B,S] and has
        no default.  With random_actions no tensor is looked at."""
        flags = (_abi.STEP_RANDOM_ACTIONS if random_actions else 0) | (_abi.STEP_AUTO_RESET if auto_reset else 0)
        shape = (self.batch_size, self.S)
        ptr = rank = None
        if not random_actions:
            if actions is None:
                if n_steps is not None:
                    raise ValueError("a rollout takes its actions from a tape int8 [n_steps,B,S] or from random_actions=True")
                actions = self.actions
            ptr = self._tensor_arg("actions", actions, (torch.int8,), shape if n_steps is None else (n_steps,) + shape)
        if act_rank is not None:
            if random_actions:
                raise ValueError("act_rank cannot be combined with random_actions")
            rank = self._tensor_arg("act_rank", act_rank, (torch.uint8,), shape)
        return flags, ptr, rank

    _TRAJECTORY_DTYPES = {"reward": (torch.float64,), "next_row": (torch.int16,), "in_use": (torch.bool, torch.uint8),
                          "terminated": (torch.bool, torch.uint8), "truncated": (torch.bool, torch.uint8),
                          "values": (torch.float64, torch.float32)}

    def _trajectory_args(self, **tensors):
        """The [T,B,S] tensors of record() / backward(), checked in the order given; `reward` sets T >= 1.  Returns (T,B,S)."""
        reward = tensors["reward"]
        if reward.dim() != 3 or reward.shape[0] < 1 or tuple(reward.shape[1:]) != (self.batch_size, self.S):
            raise ValueError(f"reward must be [T,{self.batch_size},{self.S}] with T >= 1, not {tuple(reward.shape)}")
        shape = tuple(reward.shape)
        for name, x in tensors.items():
            self._tensor_arg(name, x, self._TRAJECTORY_DTYPES[name], shape)
        return shape

    # ------------------------------------------------------------------
    def set_seeds(self, seed):
        """Env b gets Philox key ``seed + b`` (or the given per-env array)."""
        if np.isscalar(seed):
            seeds = (np.arange(self.batch_size, dtype=np.uint64) + np.uint64(int(seed) & (2 ** 64 - 1)))
        else:
            seeds = np.asarray(seed).astype(np.uint64).reshape(self.batch_size)
        self.env_seed.copy_(torch.from_numpy(seeds.view(np.int64)))

    def reset(self, seed=None, episode=0):
        """reset() of every env with on-device Philox placement (predpreygrass_rllib_env.py:129-217)."""
        if seed is not None:
            self.set_seeds(seed)
        self._check(self._lib.ppg_reset(self._handle, None, int(episode), self._stream()), "ppg_reset")
        return self

    def _placement_arrays(self, pred_xy, prey_xy, grass_xy):
        """set_placement's three arguments as int64 arrays [B,n,2]: every position inside the grid, an env's grass cells all different."""
        B, G = self.batch_size, self.grid_size
        pred = np.asarray(pred_xy, dtype=np.int64).reshape(B, self.P0, 2)
        prey = np.asarray(prey_xy, dtype=np.int64).reshape(B, self.Q0, 2)
        grass = np.asarray(grass_xy, dtype=np.int64).reshape(B, self.n_grass, 2)
        for a in (pred, prey, grass):
            if a.size and (a.min() < 0 or a.max() >= G):
                raise ValueError("position outside the grid")
        gcell = grass[..., 0] * G + grass[..., 1]
        for b in range(B):
            if len(np.unique(gcell[b])) != self.n_grass:
                raise ValueError("grass positions must be unique")
        return pred, prey, grass

    def set_placement(self, pred_xy, prey_xy, grass_xy, episode=0):
        """reset() with a given placement (arrays [B,P0,2], [B,Q0,2], [B,n_grass,2] of (x, y)):
        writes the initial state (predpreygrass_rllib_env.py:138-212) and computes the observations."""
        # the tables are built by the library (`ppg_reset_from_state`: row tables, OWNS bits in id order, grass table, env words,
        # then one ppg_observe launch)
        arrays = [np.ascontiguousarray((a[..., 0] << 8 | a[..., 1]).astype(np.uint16))
                  for a in self._placement_arrays(pred_xy, prey_xy, grass_xy)]
        init = _abi.PpgInitState()
        init.pred_xy, init.prey_xy, init.grass_xy = (a.ctypes.data for a in arrays)
        init.episode = int(episode)
        self._check(self._lib.ppg_reset_from_state(self._handle, C.byref(init), self._stream()), "ppg_reset_from_state", value_error=True)
        return self

    def set_wave_plan(self, waves=0, helper_min_rows=0, coop_envs=0):
        """Scheduling override (tests, A/B tools; results never depend on it): wavefronts per workgroup of the step kernel
        (0 = automatic), the row count from which helper wavefronts stay, envs per workgroup of the cooperative kernels
        (`ppg_set_wave_plan`)."""
        self._check(self._lib.ppg_set_wave_plan(self._handle, int(waves), int(helper_min_rows), int(coop_envs)), "ppg_set_wave_plan")
        return self

    def wave_plan(self):
        """(wavefronts per workgroup, helper_min_rows, envs per workgroup) ppg_step uses right now."""
        w, m, e = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.ppg_get_wave_plan(self._handle, C.byref(w), C.byref(m), C.byref(e)), "ppg_get_wave_plan")
        return w.value, m.value, e.value

    def step_kernel_name(self) -> str:
        return self._lib.ppg_step_kernel_name(self._handle).decode()

    def rebalance(self, stream=None):
        """Scheduling only (results are unaffected): let envs with many agents start first so that the observation
        writing is spread evenly over the CUs; call every few dozen steps (`ppg_rebalance`)."""
        self._check(self._lib.ppg_rebalance(self._handle, self._stream(stream)), "ppg_rebalance")
        return self

    def set_resident_envs(self, n: int, stream=None):
        """Cache policy only (results are unaffected): the cooperative step kernels write the observation rows of envs with index
        >= n with non-temporal stores, so that the rows of envs 0 .. n-1 stay in the Infinity Cache from step to step
        (`ppg_set_resident_envs`; `rebalance()` computes n itself unless PPG_RESIDENT_BYTES=0)."""
        self._check(self._lib.ppg_set_resident_envs(self._handle, int(n), self._stream(stream)), "ppg_set_resident_envs")
        return self

    def resident_envs(self, stream=None) -> int:
        """The count the step kernels use (`ppg_get_resident_envs`): the batch size until `rebalance()` or `set_resident_envs()` wrote one."""
        n = C.c_int32(0)
        self._check(self._lib.ppg_get_resident_envs(self._handle, C.byref(n), self._stream(stream)), "ppg_get_resident_envs")
        return int(n.value)

    def observe(self):
        """Recompute the observations of all live rows from the current state tensors."""
        self._check(self._lib.ppg_observe(self._handle, self._stream()), "ppg_observe")
        return self

    def step(self, actions=None, random_actions=False, auto_reset=False, act_rank=None, stream=None):
        """One transition of every env (predpreygrass_rllib_env.py:219-473).

        act_rank (optional uint8 [B,S]): position of each acting row within its type's action
        sequence, for action dicts whose order differs from row order.
        stream (optional): launch on this torch.cuda.Stream instead of torch's current stream."""
        flags, ptr, rank = self._step_args(actions, random_actions, auto_reset, act_rank)
        if rank is not None:
            self._check(self._lib.ppg_step_ordered(self._handle, ptr, rank, flags, self._stream(stream)), "ppg_step_ordered")
        else:
            self._check(self._lib.ppg_step(self._handle, ptr, flags, self._stream(stream)), "ppg_step")
        return self

    # SURVEY.md section 8(b)'s spelling of the tensor API: the same calls, returning views of the buffers the kernel wrote
    def reset_batch(self, seeds=None, episode=0):
        """reset() of every env (env b seeded `seeds + b`, or one seed per env); returns (obs_pred, obs_prey)."""
        self.reset(seed=seeds, episode=episode)
        return self.obs_pred, self.obs_prey

    def step_batch(self, actions=None, **kw):
        """step() of every env; returns (obs_pred[B,Sp,C,Rp,Rp], obs_prey[B,Sq,C,Rq,Rq], reward[B,S], terminated[B,S],
        truncated[B,S], live_mask[B,S], agent_id[B,S]).  Row s of env b is in use iff live_mask[b,s]; a row that terminated in
        this call is still in use (it carries its last observation and reward) and is dropped by the next call, like the
        reference keeps a dead agent in `agents` until the next step (predpreygrass_rllib_env.py:222-225,459-461)."""
        self.step(actions, **kw)
        live, flags = self.live_mask(), self.row_flags
        return (self.obs_pred, self.obs_prey, self.row_reward, ((flags & _abi.ROW_DIED) != 0) & live,
                ((flags & _abi.ROW_TRUNC) != 0) & live, live, self.row_id)

    def live_mask(self):
        """Which rows are in use: bool [B,S] on the device, nothing read back -- row r < pred_capacity iff r < the env's predator row
        count, row pred_capacity + j iff j < its prey row count (a count outside [0, capacity] acts as if clamped to it)."""
        n_pred = self.env_state[:, _abi.ENV_N_PRED_ROWS:_abi.ENV_N_PRED_ROWS + 1]
        n_prey = self.env_state[:, _abi.ENV_N_PREY_ROWS:_abi.ENV_N_PREY_ROWS + 1]
        slot, cp = self._row_index, self.pred_capacity
        return torch.where(slot < cp, slot < n_pred, slot - cp < n_prey)

    def rollout(self, n_steps, actions=None, random_actions=False, auto_reset=False, stream=None):
        """`n_steps` transitions in ONE kernel launch (state stays on chip between steps): the same result
        as `n_steps` calls of step().  Actions come from the device-side uniform random policy
        (`random_actions=True`) or from an action tape `actions` int8 [n_steps, B, S].
        Second generation: the fused form of the cooperative step kernel (the handle's wave plan must be cooperative with four waves --
        the default on a full GPU, else `set_wave_plan(4, 0, 2)`; not for the walls variant); the reproduction uniforms come from the
        device's Philox streams."""
        flags, ptr, _ = self._step_args(actions, random_actions, auto_reset, n_steps=n_steps)
        self._check(self._lib.ppg_rollout(self._handle, int(n_steps), ptr, flags, self._stream(stream)), "ppg_rollout")
        return self

    def link(self, stream=None):
        """Rows of this call's output <-> rows of the output the previous link() saw (`ppg_link`, include/ppg.h): returns
        (prev_row, next_row), two int16 [B,S] tensors owned by the env and refilled by every call (clone what has to last).
        prev_row[b, r]: the row the agent in row r had at the previous link(), next_row[b, r]: the row the agent that stood in row r
        at the previous link() has now; -1 = none (unused row, newborn / gone, another episode, first call or first call after
        reset / set_placement / import_state).  Indices are absolute row numbers, so
        ``torch.gather(x, 1, next_row.clamp_min(0).long())`` brings a [B,S] tensor of this call into the previous call's rows.
        Several steps or a rollout(K) between two calls give the K-step maps; with no step in between every row links to itself,
        except rows still flagged NEWBORN (-1 in both maps).
        stream (optional): launch on this torch.cuda.Stream instead of torch's current stream; the two tensors are then allocated
        on that stream too, and whoever reads them from another stream orders itself behind it."""
        prev_row, next_row = self._link_tensors(stream)
        self._check(self._lib.ppg_link(self._handle, _ptr(prev_row), _ptr(next_row), self._stream(stream)), "ppg_link")
        return prev_row, next_row

    def _link_tensors(self, stream=None):
        """The env's (prev_row, next_row) of link() / record(), allocated on first use."""
        if self._link_rows is None:
            self._link_rows = _alloc_on(self.device, stream, lambda: tuple(
                torch.full((self.batch_size, self.S), -1, dtype=torch.int16, device=self.device) for _ in range(2)))
        return self._link_rows

    def record(self, reward, in_use, terminated, truncated, next_row, t, stream=None):
        """link() plus the stores that keep this call's output as step t of a trajectory, in ONE launch (`ppg_record`,
        include/ppg.h: the elements written are stated there).  The five buffers are contiguous [T,B,S] tensors on the env's device,
        the inputs of backward(): reward float64, in_use / terminated / truncated bool (or uint8), next_row int16.
        t: an int in [0, T), or a one-element int32 tensor on the env's device that the kernel reads when it runs (a captured
        step + record can then be replayed while the graph counts the tensor up); if that word is outside [0, T) the call is
        link() and writes no buffer.  Returns link()'s (prev_row, next_row): the env's own tensors, written exactly as by link().
        stream (optional): as in link()."""
        shape = self._trajectory_args(reward=reward, in_use=in_use, terminated=terminated, truncated=truncated, next_row=next_row)
        step, on_device = self._step_index(t, shape[0])
        flags = _abi.RECORD_STEP_ON_DEVICE if on_device else 0
        buf = _abi.PpgRecordBuffers(shape[0], reward.data_ptr(), in_use.data_ptr(), terminated.data_ptr(), truncated.data_ptr(),
                                    next_row.data_ptr())
        prev_row, link_next = self._link_tensors(stream)
        self._check(self._lib.ppg_record(self._handle, C.byref(buf), step, flags, _ptr(prev_row), _ptr(link_next),
                                         self._stream(stream)), "ppg_record")
        return prev_row, link_next

    def _step_index(self, t, T):
        """The step argument of record() / record_obs(): (value or device address, whether the kernel reads it on the device)."""
        if isinstance(t, torch.Tensor):
            if t.dtype != torch.int32 or t.numel() != 1 or t.device != self.device:
                raise ValueError(f"t must be an int or a one-element int32 tensor on {self.device}")
            return t.data_ptr(), True
        step = int(t)
        if not 0 <= step < T:
            raise ValueError(f"t = {step} is outside [0, {T})")
        return step, False

    def _store_args(self, store):
        """What record_obs(), record_logp() and backward_samples() share of a sample store: (the `PpgObsStore` with `horizon`, `slot`
        and `capacity[2]` filled, the anchor address).  Each call refuses what only it knows first (a flag, a missing tensor list, a
        tuple that is no pair); then the arguments are checked in ONE order: `store.slot`, the capacities, the per-species tensors --
        predators then prey, per species in the order of the struct's fields --, `store.cursor`, logits or values, the step, `actions`.
        The anchor is `store.slot`, which is never empty: the address given for an EMPTY tensor, which has none (capacity 0, nothing is
        addressed through it)."""
        T = int(store.horizon)
        st = _abi.PpgObsStore()
        st.horizon = T
        st.slot = anchor = self._tensor_arg("store.slot", store.slot, (torch.int32,), (T, self.batch_size, self.S)).value
        for s in (0, 1):
            capacity = int(store.capacity[s])
            if capacity < 0:
                raise ValueError(f"store.capacity[{s}] = {capacity} < 0")
            st.capacity[s] = capacity
        return st, anchor

    def _rows_arg(self, name, x, dtypes, shape, capacity, anchor, noun="rows"):
        """The address of a per-species tensor [rows >= capacity, *shape] of a sample store (or the anchor: see _store_args)."""
        ptr = self._tensor_arg(name, x, dtypes, (None,) + shape)
        if x.shape[0] < capacity:
            raise ValueError(f"{name} has {x.shape[0]} {noun}, fewer than the capacity {capacity}")
        return ptr.value or anchor

    def record_obs(self, store, t, actions=None, f32=False, stream=None):
        """Append the observation rows in use of this call's output, as step t, to a compact per-species sample store
        (`ppg_record_obs`, include/ppg.h: order, overflow and the elements written are stated there), in two launches.
        store: a `trajectory.ObservationStore`, or any object with its tensors -- `horizon` T, `capacity` (n_pred, n_prey),
        `obs` [2] of [rows >= capacity, C, R, R] in the env's observation dtype (float32 with f32=True on a float64 env), `sample` [2]
        int32 [rows], `action` None or [2] int8 [rows], `slot` int32 [T,B,S], `cursor` int64 [4].
        t: as in record().  actions: the int8 [B,S] tensor the env's last step was given (they answer the observations stored by the
        previous record_obs()), or None -- no actions are stored (device-drawn random actions).
        stream (optional): launch on this torch.cuda.Stream instead of torch's current stream."""
        if f32 and self.obs_dtype == torch.bfloat16:
            raise ValueError("f32=True is for float64 (and float32) observations, not bfloat16")
        if actions is not None and store.action is None:
            raise ValueError("actions were given but the store keeps none")
        dtype = torch.float32 if f32 and self.obs_dtype == torch.float64 else self.obs_dtype
        st, anchor = self._store_args(store)
        for s, src in enumerate((self.obs_pred, self.obs_prey)):
            capacity = st.capacity[s]
            st.obs[s] = self._rows_arg(f"store.obs[{s}]", store.obs[s], (dtype,), tuple(src.shape[2:]), capacity, anchor)
            st.sample[s] = self._rows_arg(f"store.sample[{s}]", store.sample[s], (torch.int32,), (), capacity, anchor)
            if store.action is not None:
                st.action[s] = self._rows_arg(f"store.action[{s}]", store.action[s], (torch.int8,), (), capacity, anchor)
        st.cursor = self._tensor_arg("store.cursor", store.cursor, (torch.int64,), (4,)).value
        step, on_device = self._step_index(t, st.horizon)
        flags = (_abi.OBS_STEP_ON_DEVICE if on_device else 0) | (_abi.OBS_F32 if f32 else 0)
        act = None if actions is None else self._tensor_arg("actions", actions, (torch.int8,), (self.batch_size, self.S))
        self._check(self._lib.ppg_record_obs(self._handle, C.byref(st), step, flags, act, self._stream(stream)), "ppg_record_obs")
        return store

    def record_logp(self, store, t, logits, actions=None, stream=None):
        """What the behaviour policy thought of the samples that record_obs() stored as step t: `store.logp[s][k]` = log pi(a|o) of the
        action taken from slot k, `store.entropy[s][k]`, `store.dist[s][k]` = the logits (`ppg_record_logp`, include/ppg.h: the
        arithmetic and the elements written are stated there), in two launches, nothing read back.  Call it behind
        `FusedPolicy.act(..., logits=...)` and in front of the next step().
        store: a `trajectory.ObservationStore(..., logp=(A_pred, A_prey))`, or any object with `horizon` T, `capacity`, `slot` int32
        [T,B,S], `n_actions` (A_pred, A_prey), `logp` [2] float32 [rows >= capacity], `entropy` None or [2] likewise, `dist` None or [2]
        float32 [rows, A_s].
        t: the recorded step the env's current output was stored as -- an int in [0, T); or the one-element int32 tensor record()
        takes, which already names the NEXT step: the kernels then use its value minus one and write nothing if that is outside [0, T).
        logits: (logits_pred, logits_prey), float32 [B * capacity_s, A_s] as `FusedPolicy.act()` fills them; either may be None -- that
        species is skipped.  actions: the int8 [B,S] tensor act() filled (default: `env.actions`).
        stream (optional): launch on this torch.cuda.Stream instead of torch's current stream."""
        if getattr(store, "logp", None) is None:
            raise ValueError("the store keeps no log-probabilities: ObservationStore(..., logp=(A_pred, A_prey))")
        if len(logits) != 2:
            raise ValueError("logits must be the pair (logits_pred, logits_prey); either may be None")
        st, anchor = self._store_args(store)
        out, f32, lg = _abi.PpgLogpStore(), (torch.float32,), [None, None]
        for s, cap in enumerate((self.pred_capacity, self.prey_capacity)):
            capacity, A = st.capacity[s], int(store.n_actions[s])
            if not 1 <= A <= 32:
                raise ValueError(f"store.n_actions[{s}] = {A} is outside 1..32")
            out.n_actions[s] = A
            out.logp[s] = self._rows_arg(f"store.logp[{s}]", store.logp[s], f32, (), capacity, anchor)
            if store.entropy is not None:
                out.entropy[s] = self._rows_arg(f"store.entropy[{s}]", store.entropy[s], f32, (), capacity, anchor)
            if store.dist is not None:
                out.dist[s] = self._rows_arg(f"store.dist[{s}]", store.dist[s], f32, (A,), capacity, anchor)
            if logits[s] is not None:
                lg[s] = self._tensor_arg(f"logits[{s}]", logits[s], f32, (self.batch_size * cap, A))
        step, on_device = self._step_index(t, st.horizon)
        act = self._tensor_arg("actions", self.actions if actions is None else actions, (torch.int8,), (self.batch_size, self.S))
        self._check(self._lib.ppg_record_logp(self._handle, C.byref(st), C.byref(out), step, _abi.LOGP_STEP_ON_DEVICE if on_device else 0,
                                              lg[0], lg[1], act, self._stream(stream)), "ppg_record_logp")
        return store

    def backward(self, reward, next_row, in_use, terminated, truncated, gamma, lam=1.0, values=None, returns=True,
                 advantages=None, stream=None):
        """Discounted returns and generalised advantages over a recorded horizon in ONE launch (`ppg_backward`, include/ppg.h:
        the recursion and its cases are stated there).  All inputs are contiguous [T,B,S] tensors on the env's device: reward
        float64, next_row int16 (`link()`'s next_row of the call after step t), in_use / terminated / truncated bool (or uint8
        0 / 1), values float64 or float32 (only needed for advantages).  Returns (G, A), float64 [T,B,S] each, newly allocated;
        the one not asked for (`returns=False`; `advantages` defaults to "values were given") is None.  The env's state is not
        touched: the handle only supplies B, S and the device.
        stream (optional): as in link() -- the launch and the allocation of the outputs go to that stream."""
        want_a = (values is not None) if advantages is None else bool(advantages)
        if not returns and not want_a:
            raise ValueError("backward: neither returns nor advantages asked for")
        if want_a and values is None:
            raise ValueError("backward: advantages need values")
        shape = self._trajectory_args(reward=reward, next_row=next_row, in_use=in_use, terminated=terminated, truncated=truncated,
                                      **({"values": values} if want_a else {}))
        G, A = _alloc_on(self.device, stream, lambda: tuple(
            torch.empty(shape, dtype=torch.float64, device=self.device) if want else None for want in (returns, want_a)))
        self._check(self._lib.ppg_backward(self._handle, shape[0], _ptr(reward), _ptr(next_row), _ptr(in_use), _ptr(terminated),
                                           _ptr(truncated), _ptr(values) if want_a else None,
                                           _abi.F32 if want_a and values.dtype == torch.float32 else _abi.F64,
                                           float(gamma), float(lam), _ptr(G), _ptr(A), self._stream(stream)), "ppg_backward")
        return G, A

    def backward_samples(self, store, reward, next_row, in_use, terminated, truncated, gamma, lam=1.0, values=(None, None),
                         advantages=True, returns=True, stats=False, stream=None):
        """backward() from and into SAMPLE order, in ONE launch (`ppg_backward_samples`, include/ppg.h: the recursion, the rows stored
        and the order of the sums are stated there): the critic's values are read per sample, `values[s][k]` of slot k of species s
        through `store.slot`, and the advantage and return of every stored row are written to its slot, rounded once to float32.
        store: a `trajectory.ObservationStore`, or any object with `horizon` (>= T), `capacity` (n_pred, n_prey) and `slot` int32
        [horizon,B,S]; nothing else of it is looked at.  reward ... truncated: backward()'s [T,B,S] tensors.
        values: (v_pred, v_prey), float64 or float32 [rows >= capacity[s]] of ONE dtype; None: V = 0 for that species.
        Returns (advantages, returns, stats): two pairs of float32 [capacity[s]] tensors (None where not asked for), newly allocated
        and zero in every slot no stored row of the T steps has; stats (stats=True, needs advantages): float64 [B,2,3], per env and
        species {count, sum A, sum A * A} over the stored rows from the unrounded float64 A -- `stats.sum(0)` are the batch's.
        stream (optional): as in backward() -- the launch and the allocation of the outputs go to that stream."""
        if not returns and not advantages:
            raise ValueError("backward_samples: neither returns nor advantages asked for")
        if stats and not advantages:
            raise ValueError("backward_samples: stats need advantages")
        if len(values) != 2:
            raise ValueError("values must be the pair (v_pred, v_prey); either may be None")
        shape = self._trajectory_args(reward=reward, next_row=next_row, in_use=in_use, terminated=terminated, truncated=truncated)
        if shape[0] > int(store.horizon):
            raise ValueError(f"{shape[0]} steps, but the store's horizon is {int(store.horizon)}")
        given = [v for v in values if v is not None]
        if any(v.dtype != given[0].dtype for v in given):
            raise ValueError("values of the two species must have one dtype")
        st, anchor = self._store_args(store)
        tg, capacity = _abi.PpgSampleTargets(), tuple(st.capacity)
        for s, v in enumerate(values):
            if v is not None:
                tg.values[s] = self._rows_arg(f"values[{s}]", v, self._TRAJECTORY_DTYPES["values"], (), capacity[s], anchor, "elements")

        def outputs():
            pair = lambda: [torch.zeros((n,), dtype=torch.float32, device=self.device) for n in capacity]
            return (pair() if advantages else None, pair() if returns else None,
                    torch.empty((self.batch_size, 2, 3), dtype=torch.float64, device=self.device) if stats else None)
        adv, ret, moments = _alloc_on(self.device, stream, outputs)
        for s in (0, 1):   # (the outputs of a species of capacity 0 are empty: anchored like its inputs)
            if adv is not None:
                tg.advantage[s] = adv[s].data_ptr() or anchor
            if ret is not None:
                tg.returns[s] = ret[s].data_ptr() or anchor
        if moments is not None:
            tg.stats = moments.data_ptr()
        self._check(self._lib.ppg_backward_samples(self._handle, shape[0], _ptr(reward), _ptr(next_row), _ptr(in_use), _ptr(terminated),
                                                   _ptr(truncated), C.byref(st), C.byref(tg),
                                                   _abi.F32 if given and given[0].dtype == torch.float32 else _abi.F64,
                                                   float(gamma), float(lam), self._stream(stream)), "ppg_backward_samples")
        return adv, ret, moments

    def ppo_loss(self, logits, action, logp, advantage, index=None, values=None, value_target=None, dist=None, adv_norm=None,
                 clip=0.3, vf_clip=10.0, vf_coeff=1.0, ent_coeff=0.0, kl_coeff=0.0, stream=None):
        """The gradients and per-chunk sums of PPO's clipped loss over one minibatch of ONE species, in two launches (`ppg_ppo_loss`,
        include/ppg.h: validity, the arithmetic line by line, the columns of `partial` and the order of its sums are stated there).
        logits: float32 [M,A], the learner's new logits, row i for slot `index[i]`; index: int32 [M] or None (slot i); values: float32
        [M] or None (no value term).  action int8 [capacity], logp float32 [capacity], dist float32 [capacity,A] or None, advantage
        float32 [>= capacity], value_target float32 [>= capacity] (given exactly when values is): the columns of a sample store and of
        backward_samples(); `capacity` is action's length.  adv_norm: float64 [2] {shift, scale} on the device or None.
        Returns (grad_logits float32 [M,A], grad_values float32 [M] or None, partial float64 [ceil(M / 1024), 8]), newly allocated and
        written completely; `partial.sum(0)` = {n, sum surr, sum vfc, sum vf, sum H, sum KL, clipped rows, sum (logp_old - logp_new)}
        over the valid rows.  The env's state is not touched.
        stream (optional): as in backward() -- the launches and the allocation of the outputs go to that stream."""
        f32 = (torch.float32,)
        if logits.dim() != 2 or logits.shape[0] < 1 or not 1 <= logits.shape[1] <= 32:
            raise ValueError(f"logits must be [M,A] with M >= 1 and A in 1..32, not {tuple(logits.shape)}")
        M, A = (int(n) for n in logits.shape)
        mb = _abi.PpgPpoBatch()
        mb.M, mb.A = M, A
        mb.logits = anchor = self._tensor_arg("logits", logits, f32, (M, A)).value
        if index is not None:
            if not isinstance(index, torch.Tensor) or index.dtype != torch.int32:
                raise ValueError(f"index must have dtype=torch.int32 (the slot words of the store), not {getattr(index, 'dtype', type(index))}")
            mb.index = self._tensor_arg("index", index, (torch.int32,), (M,)).value
        if (values is None) != (value_target is None):
            raise ValueError("values and value_target come together: both tensors, or both None")
        if values is not None:
            mb.values = self._tensor_arg("values", values, f32, (M,)).value
        if action.dim() != 1:
            raise ValueError(f"action must be [capacity], not {tuple(action.shape)}")
        capacity = mb.capacity = int(action.shape[0])
        mb.action = self._rows_arg("action", action, (torch.int8,), (), capacity, anchor)
        mb.logp = self._rows_arg("logp", logp, f32, (), capacity, anchor, "elements")
        if dist is not None:
            mb.dist = self._rows_arg("dist", dist, f32, (A,), capacity, anchor)
        mb.advantage = self._rows_arg("advantage", advantage, f32, (), capacity, anchor, "elements")
        if value_target is not None:
            mb.value_target = self._rows_arg("value_target", value_target, f32, (), capacity, anchor, "elements")
        if adv_norm is not None:
            mb.adv_norm = self._tensor_arg("adv_norm", adv_norm, (torch.float64,), (2,)).value
        mb.clip, mb.vf_clip, mb.vf_coeff, mb.ent_coeff, mb.kl_coeff = (float(x) for x in (clip, vf_clip, vf_coeff, ent_coeff, kl_coeff))
        G = (M + _abi.PPO_CHUNK - 1) // _abi.PPO_CHUNK
        grad_logits, grad_values, partial = _alloc_on(self.device, stream, lambda: (
            torch.empty((M, A), dtype=torch.float32, device=self.device),
            torch.empty((M,), dtype=torch.float32, device=self.device) if values is not None else None,
            torch.empty((G, 8), dtype=torch.float64, device=self.device)))
        self._check(self._lib.ppg_ppo_loss(self._handle, C.byref(mb), _ptr(grad_logits), _ptr(grad_values), _ptr(partial),
                                           self._stream(stream)), "ppg_ppo_loss", value_error=True)
        return grad_logits, grad_values, partial

    # ------------------------------------------------------------------
    # the policy networks' training pass (`ppg_net_forward` / `ppg_net_backward`, include/ppg.h; csrc/ppg_net.h)
    _OBS_DTYPES = {torch.float64: 0, torch.float32: 1, torch.bfloat16: 2}

    def _net_spec(self, net, what="parameter"):
        """`ppg_policy_spec` of a `policy.PolicyNet` whose parameters the kernels read in place: float32, contiguous, on the env's device."""
        from .policy import FusedPolicy   # (policy imports this module)
        names = {id(p): n for n, p in net.named_parameters()}
        return FusedPolicy._spec(net, lambda p: self._tensor_arg(f"{what} {names.get(id(p), '?')}", p, (torch.float32,), tuple(p.shape)).value)

    @staticmethod
    def _net_grad_spec(net, base):
        """The `grads` argument of ppg_net_backward: net's shape with pointers into a flat float32 buffer at address `base`."""
        from .policy import FusedPolicy
        offsets = iter(net_grad_offsets(net))
        return FusedPolicy._spec(net, lambda p: base + 4 * next(offsets))

    def net_bytes(self, net, M, groups=0):
        """(workspace bytes, partial bytes, n_params, TS) of net_forward() / net_backward() for a minibatch of M rows (`ppg_net_bytes`: no
        device involved).  The flat gradient buffer holds conv0.weight, conv0.bias, ..., fc0.weight, fc0.bias, ... in that order."""
        from .policy import FusedPolicy
        out = (C.c_uint64 * 4)()
        shape = FusedPolicy._spec(net, lambda p: None)   # (the weight pointers are not read: the net may live anywhere)
        rc = self._lib.ppg_net_bytes(C.byref(shape), int(M), int(groups), C.byref(out))
        if rc != 0:
            raise ValueError(self._lib.ppg_last_error(None).decode())
        return tuple(int(x) for x in out)

    def _net_batch(self, net, obs, index, M, groups, out, workspace):
        """The `ppg_net_batch` both calls take, after the checks both make."""
        if obs.dim() != 4 or tuple(obs.shape[1:]) != (net.obs_channels, net.obs_range, net.obs_range):
            raise ValueError(f"obs must be [capacity,{net.obs_channels},{net.obs_range},{net.obs_range}], not {tuple(obs.shape)}")
        mb = _abi.PpgNetBatch()
        mb.obs = self._tensor_arg("obs", obs, tuple(self._OBS_DTYPES), tuple(obs.shape)).value
        mb.obs_dtype, mb.capacity, mb.groups = self._OBS_DTYPES[obs.dtype], int(obs.shape[0]), int(groups)
        if index is not None:
            if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1:
                raise ValueError(f"index must be an int32 tensor [M] (the slot words of the store), not {getattr(index, 'dtype', type(index))}")
            mb.index = self._tensor_arg("index", index, (torch.int32,), (int(index.shape[0]),)).value
        mb.M = int(M if M is not None else index.shape[0] if index is not None else obs.shape[0])
        if index is not None and mb.M != index.shape[0]:
            raise ValueError(f"M = {mb.M}, but index has {index.shape[0]} rows")
        if out is not None:   # (backward writes no out)
            mb.out = self._tensor_arg("out", out, (torch.float32,), (mb.M, net.n_actions)).value
        if workspace.dim() != 1:
            raise ValueError(f"workspace must be a flat float32 tensor, not {tuple(workspace.shape)}")
        mb.workspace = self._tensor_arg("workspace", workspace, (torch.float32,), (None,)).value
        mb.workspace_bytes = workspace.numel() * 4
        return mb

    def net_forward(self, net, obs, index=None, M=None, groups=0, out=None, workspace=None, stream=None):
        """`net`'s float32 forward pass over the minibatch rows `obs[index]` in ONE launch (`ppg_net_forward`, include/ppg.h: rows, tiles
        and the arithmetic are stated there).  net: a `policy.PolicyNet` whose parameters are float32 on the env's device (they are
        read where they lie, when the kernel runs); obs: contiguous [capacity,C,R,R] float64 / float32 / bfloat16; index: int32 [M] or
        None (rows 0 .. M - 1; M defaults to the capacity).  A row whose slot is outside [0, capacity) gets +0.0 and nothing of it is
        read.  groups: 0, or the number of workgroups (tests, A/B runs).
        Returns (out float32 [M,n_actions], workspace): the flat float32 tensor of activations that net_backward() of the same
        minibatch reads -- both newly allocated unless given.
        stream (optional): as in backward() -- the launch and the allocations go to that stream."""
        rows = int(M if M is not None else index.shape[0] if isinstance(index, torch.Tensor) else obs.shape[0])
        need = self.net_bytes(net, rows, groups)
        out, workspace = _alloc_on(self.device, stream, lambda: (
            torch.empty((rows, net.n_actions), dtype=torch.float32, device=self.device) if out is None else out,
            torch.empty((need[0] // 4,), dtype=torch.float32, device=self.device) if workspace is None else workspace))
        mb = self._net_batch(net, obs, index, rows, groups, out, workspace)
        self._check(self._lib.ppg_net_forward(self._handle, C.byref(self._net_spec(net)), C.byref(mb), self._stream(stream)),
                    "ppg_net_forward", value_error=True)
        return out, workspace

    def net_backward(self, net, obs, index, grad_out, workspace, M=None, groups=0, grads=None, partial=None, stream=None):
        """The gradients of `net`'s parameters for d loss / d out = grad_out, in TWO launches (`ppg_net_backward`): per workgroup partial
        sums without atomics, then their sum in a fixed order -- the same bits from run to run.  obs, index, M, groups and workspace:
        those of the net_forward() call whose activations `workspace` holds; grad_out float32 [M,n_actions] (rows that are selections
        are not read).  grads: a flat float32 tensor [n_params] to write into, partial: a flat float32 tensor of net_bytes()[1] / 4
        elements -- both newly allocated unless given.  Returns (grads, partial); `net_grad_views(net, grads)` are the per-parameter
        views, in the order conv0.weight, conv0.bias, ..., fc0.weight, fc0.bias, ...
        stream (optional): as in net_forward()."""
        rows = int(M if M is not None else index.shape[0] if isinstance(index, torch.Tensor) else obs.shape[0])
        need = self.net_bytes(net, rows, groups)
        grads, partial = _alloc_on(self.device, stream, lambda: (
            torch.empty((need[2],), dtype=torch.float32, device=self.device) if grads is None else grads,
            torch.empty((need[1] // 4,), dtype=torch.float32, device=self.device) if partial is None else partial))
        mb = self._net_batch(net, obs, index, rows, groups, None, workspace)
        g = self._tensor_arg("grad_out", grad_out, (torch.float32,), (rows, net.n_actions))
        base = self._tensor_arg("grads", grads, (torch.float32,), (need[2],)).value
        if partial.dim() != 1:
            raise ValueError(f"partial must be a flat float32 tensor, not {tuple(partial.shape)}")
        part = self._tensor_arg("partial", partial, (torch.float32,), (None,))
        gspec = self._net_grad_spec(net, base)
        self._check(self._lib.ppg_net_backward(self._handle, C.byref(self._net_spec(net)), C.byref(mb), g, C.byref(gspec), part,
                                               partial.numel() * 4, self._stream(stream)), "ppg_net_backward", value_error=True)
        return grads, partial

    def export_grid(self):
        """grid_world_state of every env: float64 [B,4,G,G] (predpreygrass_rllib_env.py:124)."""
        G = self.grid_size
        out = torch.empty((self.batch_size, 4, G, G), dtype=torch.float64, device=self.device)
        self._check(self._lib.ppg_export_grid(self._handle, _ptr(out), self._stream()), "ppg_export_grid")
        return out

    def export_state(self, b=0) -> bytes:
        """Versioned image of env b's state (`ppg_export_state`): row tables, env words, Philox key, grass table --
        what get_state_snapshot of the reference captures (predpreygrass_rllib_env.py:768-786), as one POD blob."""
        size = C.c_uint64(int(self._lib.ppg_state_bytes(self._handle)))
        blob = C.create_string_buffer(size.value)
        self._check(self._lib.ppg_export_state(self._handle, int(b), blob, C.byref(size), self._stream()), "ppg_export_state")
        return blob.raw[: size.value]

    def import_state(self, blob: bytes, b=0):
        """Write an image from `export_state` into env b (`ppg_import_state`, predpreygrass_rllib_env.py:788-804); the
        geometry of the handle it came from must match.  Call `observe()` afterwards for the observations."""
        buf = C.create_string_buffer(bytes(blob), len(blob))
        self._check(self._lib.ppg_import_state(self._handle, int(b), buf, len(blob), self._stream()), "ppg_import_state", value_error=True)
        return self

    # ------------------------------------------------------------------
    # the dict classes' host traffic: ONE copy each way per call (`ppg_fetch`, include/ppg.h)
    def _fetch_fields(self):
        """(name, numpy dtype, elements) of an env's record in a fetch image: the state image's field order (include/ppg.h)."""
        S, NG = self.S, self.grass_capacity
        return [("row_xy", "<i2", S), ("row_energy", "<f8", S), ("row_id", "<i4", S), ("row_key", "<i4", S), ("row_cumrew", "<f8", S),
                ("row_flags", "u1", S), ("row_reward", "<f8", S), ("row_parent", "<i4", S), ("env_state", "<i4", _abi.ENV_WORDS),
                ("env_seed", "<i8", 1), ("grass_xy", "<i2", NG), ("grass_energy", "<f8", NG)]

    def _host_buffer(self, nbytes, dtype=torch.uint8):
        """Host memory the library copies into / out of: pinned on a GPU (the copy is then asynchronous), plain for the CPU test build."""
        if self.device.type == "cuda":
            return torch.empty((nbytes,), dtype=dtype).pin_memory()
        return torch.empty((nbytes,), dtype=dtype)

    def fetch(self, env0=0, n=None):
        """What the last call returned for envs [env0, env0 + n), on the host after ONE gather launch, ONE device->host copy and ONE
        stream synchronisation (`ppg_fetch`): (tables, obs_pred, obs_prey) -- tables[name] is the [n, ...] slice of every state tensor
        (a copy), obs_pred[i] / obs_prey[i] the observation blocks IN USE of env env0 + i as arrays [rows, C, R, R] (views into the
        staging buffer: valid until the next fetch)."""
        if self.obs_dtype not in (torch.float64, torch.float32):
            raise RuntimeError("fetch() hands observations to numpy: float64 or float32 rows")
        n = self.batch_size - env0 if n is None else int(n)
        if getattr(self, "_fetch_host", None) is None:
            guess = int(self._lib.ppg_fetch_bytes(self._handle, n, n * min(self.pred_capacity, 24), n * min(self.prey_capacity, 96)))
            self._fetch_host = self._host_buffer(guess)
        for _ in range(3):
            cap = self._fetch_host.numel()
            rc = self._lib.ppg_fetch(self._handle, int(env0), n, C.c_void_p(self._fetch_host.data_ptr()), cap, self._stream())
            if rc == -1 and cap < int(self._lib.ppg_fetch_bytes(self._handle, n, 0, 0)):   # (more envs than the buffer was sized for)
                self._fetch_host = self._host_buffer(int(self._lib.ppg_fetch_bytes(self._handle, n, n * 24, n * 96)))
                continue
            self._check(rc, "ppg_fetch")
            buf = self._fetch_host.numpy()
            H = _abi.PpgFetchHeader.from_buffer(buf[:64])
            if H.magic != _abi.FETCH_MAGIC or H.version != _abi.FETCH_VERSION:
                raise RuntimeError("ppg_fetch returned an image of another version")
            if not H.overflow:
                break
            self._fetch_host = self._host_buffer(int(H.bytes_used) * 3 // 2)
        else:
            raise RuntimeError("ppg_fetch: the image keeps overflowing")
        rec_bytes, bp, bq = int(H.record_bytes), int(H.blk_pred_bytes), int(H.blk_prey_bytes)
        rec = np.array(buf[64:64 + n * rec_bytes]).reshape(n, rec_bytes)   # (a copy: the tables outlive the staging buffer's next use)
        if getattr(self, "_fetch_layout", None) is None:   # (name, dtype, byte offset, bytes) of every field of a record, once
            lay, off = [], 0
            for name, dt, count in self._fetch_fields():
                nb = np.dtype(dt).itemsize * count
                lay.append((name, dt, off, nb))
                off += (nb + 7) // 8 * 8
            self._fetch_layout = lay
        tables = {name: rec[:, off:off + nb].view(dt) for name, dt, off, nb in self._fetch_layout}
        if "row_info" not in tables:
            tables["row_info"] = np.zeros((n, self.S), dtype=np.uint8)
        es = tables["env_state"]
        odt = np.float64 if self.obs_dtype == torch.float64 else np.float32
        pshape, qshape = tuple(self.obs_pred.shape[2:]), tuple(self.obs_prey.shape[2:])
        obs_p, obs_q, o = [], [], 64 + n * rec_bytes
        for kp, kq in zip(es[:, _abi.ENV_N_PRED_ROWS].tolist(), es[:, _abi.ENV_N_PREY_ROWS].tolist()):
            obs_p.append(buf[o:o + kp * bp].view(odt).reshape((kp,) + pshape))
            o += (kp * bp + 15) // 16 * 16
            obs_q.append(buf[o:o + kq * bq].view(odt).reshape((kq,) + qshape))
            o += (kq * bq + 15) // 16 * 16
        return tables, obs_p, obs_q

    def stage_actions(self, env=None):
        """The pinned host mirror of the action tensor (int8 numpy [B,S]) and its upload: fill `stage_actions()` rows, then
        `upload_actions()` -- ONE asynchronous host->device copy for all envs."""
        if getattr(self, "_act_host", None) is None:
            self._act_host = self._host_buffer(self.batch_size * self.S, torch.int8).view(self.batch_size, self.S)
            self._act_host.fill_(_abi.ACTION_NONE)
        a = self._act_host.numpy()
        return a if env is None else a[env]

    def upload_actions(self):
        self.actions.copy_(self._act_host, non_blocking=True)
        return self

    # ------------------------------------------------------------------
    # host views (one device->host copy each; used by tests and by white-box state surgery)
    _HOST_TABLES = ("row_xy", "row_energy", "row_id", "row_cumrew", "row_flags", "row_reward", "row_parent", "env_state",
                    "grass_xy", "grass_energy")

    def host_tables(self, b=None):
        """Small per-env tables copied to the host as numpy arrays."""
        sl = slice(None) if b is None else slice(b, b + 1)
        return {n: getattr(self, n)[sl].cpu().numpy() for n in self._HOST_TABLES}

    def records(self, b, tables=None):
        """The returned dicts of env b's last call as an ordered list of
        (name, type, row, reward, terminated, truncated) in the reference's dict order:
        predator survivors, prey survivors, predator newborns, prey newborns."""
        t = tables if tables is not None else self.host_tables(b)
        i = 0 if tables is None else b
        es = t["env_state"][i].tolist()
        nP, nQ = es[_abi.ENV_N_PRED_ROWS], es[_abi.ENV_N_PREY_ROWS]
        newP, newQ = es[_abi.ENV_N_PRED_NEW], es[_abi.ENV_N_PREY_NEW]
        cp = self.pred_capacity
        # (whole rows as Python lists once: indexing numpy scalars one by one costs more than the rest of the dict assembly)
        ids, fls, rws = t["row_id"][i].tolist(), t["row_flags"][i].tolist(), t["row_reward"][i].tolist()
        out = []
        for ty, lo, hi in ((PREDATOR, 0, nP - newP), (PREY, 0, nQ - newQ), (PREDATOR, nP - newP, nP), (PREY, nQ - newQ, nQ)):
            base, fmt = (0, "predator_%d") if ty == PREDATOR else (cp, "prey_%d")
            for r in range(lo, hi):
                fl = fls[base + r]
                out.append((fmt % ids[base + r], ty, r, rws[base + r], bool(fl & _abi.ROW_DIED), bool(fl & _abi.ROW_TRUNC)))
        return out
