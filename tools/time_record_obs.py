"""Times what storing observations and actions costs behind a recorded step, on a real MI355X: `env.record_obs()` (`ppg_record_obs`:
the rows in use appended to a compact per-species store, two launches) against its torch restatement
(`ObservationStore.record_obs_torch()`: `nonzero` plus gathers, the host waits every step) and against `ppg_pack` of the same handle --
the project's existing compacting copy of the same rows, which rewrites ONE image every step where the store appends a horizon's worth.
Per step, launch to launch, in alternating blocks within one process:

    (a) step + record()                        (b) step + record() + record_obs()
    (c) step + record() + record_obs_torch()   (d) step + ppg_pack

HIP events around blocks of `--block` steps, a warm-up block of every mode, `--reps` blocks each, median and min-max of the per-step
time; the rows stored per step, the bytes the call has to move -- sum over the rows in use of blk * (src + dst element) + S * 4 per env
+ (4 + 1) per row in use -- and the rate that gives over (b) - (a).  Before any timing the bytes of record_obs() are compared with
record_obs_torch() at the timed size.

    python tools/time_record_obs.py                        # bfloat16 and float64 handles, one child process each
    python tools/time_record_obs.py --batch 64 --reps 3 --preroll 50 --block 16   # a rehearsal at a small size

Each dtype runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is
started."""
import argparse
import ctypes as C
import statistics
import sys

from timing import alternate, fmt, run_children   # (tools/timing.py)

DTYPES = ["bfloat16", "float64"]


def child(args):
    import torch
    from predpreygrass_amd import _abi
    from predpreygrass_amd.batched import BatchedPredPreyGrass
    from predpreygrass_amd.config import config_env
    from predpreygrass_amd.trajectory import AgentTrajectories, ObservationStore
    assert torch.cuda.is_available(), "time_record_obs needs a ROCm GPU"
    dtype = getattr(torch, DTYPES[args.child])
    B, T = args.batch, args.block
    env = BatchedPredPreyGrass(config_env, batch_size=B, device="cuda:0", seed=1, obs_dtype=dtype)
    S, elem = env.S, env.obs_pred.element_size()
    blk = (env.obs_pred[0, 0].numel(), env.obs_prey[0, 0].numel())

    def step():
        env.step(random_actions=True, auto_reset=True)

    env.reset()
    for _ in range(args.preroll):   # to a stationary population
        step()
    live = env.live_mask()
    n_pred, n_prey = live[:, :env.pred_capacity].sum().item(), live[:, env.pred_capacity:].sum().item()
    # stores for one block of steps at the stationary population, with a quarter to spare (what does not fit is dropped, and reported)
    rows = (int(T * n_pred * 1.25) + B, int(T * n_prey * 1.25) + B)
    traj = AgentTrajectories(env, T)
    store, store_torch = ObservationStore(env, T, rows, actions=True), ObservationStore(env, T, rows, actions=True)
    # the results must not differ (byte for byte) before any time is worth reporting
    for t in range(min(T, 8)):
        step()
        store.record(t)
        store_torch.record_obs_torch(t)
    torch.cuda.synchronize()
    for name in ("slot", "cursor"):
        assert torch.equal(getattr(store, name), getattr(store_torch, name)), f"kernel != record_obs_torch(): {name}"
    for s in (0, 1):
        for a, b in ((store.obs[s], store_torch.obs[s]), (store.sample[s], store_torch.sample[s]), (store.action[s], store_torch.action[s])):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"kernel != record_obs_torch(): species {s}"
    assert int(store.cursor[0]) > 0 and int(store.cursor[1]) > 0, "nothing was stored"

    lib, handles = env._lib, (C.c_void_p * 1)(env._handle)
    image_bytes = int(lib.ppg_pack_bytes(env._handle, B, rows[0] // T, rows[1] // T, 0))
    image = torch.empty((image_bytes,), dtype=torch.uint8, device=env.device)

    def record(t):
        env.record(traj.reward, traj.in_use, traj.terminated, traj.truncated, traj.next_row, t)

    def block_a(n):
        for t in range(n):
            step()
            record(t)

    def block_b(n):
        store.clear()
        for t in range(n):
            step()
            record(t)
            store.record(t)

    def block_c(n):
        store_torch.clear()
        for t in range(n):
            step()
            record(t)
            store_torch.record_obs_torch(t)

    def block_d(n):
        for t in range(n):
            step()
            rc = lib.ppg_pack(handles, 1, C.c_void_p(image.data_ptr()), image_bytes, 0, env._stream())
            assert rc == 0, lib.ppg_last_error(env._handle)

    modes = [("(a) step + record()", block_a), ("(b) step + record() + record_obs()", block_b),
             ("(c) step + record() + record_obs_torch()", block_c), ("(d) step + ppg_pack", block_d)]
    counts = []
    times = alternate(modes, args.reps, T, after={modes[1][0]: lambda: counts.append(store.counts())})
    (sp, dp), (sq, dq) = counts[-1]
    stored, dropped = (sp / T, sq / T), dp + dq
    header = _abi.PpgPackHeader.from_buffer_copy(image[:64].cpu().numpy().tobytes())
    per_step = sum(stored[s] * (blk[s] * 2 * elem + 5) for s in (0, 1)) + B * S * 4
    med = {name[:3]: statistics.median(ts) for name, ts in times.items()}
    spread = {name[:3]: max(ts) - min(ts) for name, ts in times.items()}
    print(f"### B = {B}, S = {S}, {DTYPES[args.child]} observations (blocks of {blk[0]} / {blk[1]} elements), kernel {env.step_kernel_name()}; "
          f"{stored[0]:.0f} predator + {stored[1]:.0f} prey rows stored per step ({(stored[0] + stored[1]) / (B * S):.1%} of the rows), {dropped} dropped; "
          f"ppg_pack overflow {header.overflow}; µs per step, launch to launch, {args.reps} blocks of {T} steps each, median (min-max)", flush=True)
    print("| what | µs per step |\n|---|---|")
    for name, _ in modes:
        print(f"| {name} | {fmt(times[name], 1)} |", flush=True)
    cost = med["(b)"] - med["(a)"]
    print(f"record_obs() costs {cost:.1f} µs per step, record_obs_torch() {med['(c)'] - med['(a)']:.1f}, ppg_pack {med['(d)'] - med['(a)']:.1f} "
          f"(spreads: (a) {spread['(a)']:.1f}, (b) {spread['(b)']:.1f}, (c) {spread['(c)']:.1f}, (d) {spread['(d)']:.1f}); "
          f"{per_step / 1e6:.1f} MB to move per step = {per_step / cost / 1e6 if cost > 0 else float('nan'):.2f} TB/s over (b) - (a)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--block", type=int, default=128, help="steps between two events = the horizon of the stores")
    ap.add_argument("--reps", type=int, default=7, help="timed blocks per mode")
    ap.add_argument("--preroll", type=int, default=700, help="steps before anything is timed")
    ap.add_argument("--limit", type=int, default=240, help="seconds a dtype's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    passed = ["--batch", str(args.batch), "--block", str(args.block), "--reps", str(args.reps), "--preroll", str(args.preroll)]
    return run_children(__file__, len(DTYPES), passed, args.limit, lambda i: DTYPES[i])


if __name__ == "__main__":
    sys.exit(main())
