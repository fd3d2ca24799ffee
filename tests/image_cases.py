"""Cases of `ppg_pack` (csrc/ppg_pack.h) and `ppg_fetch` (csrc/ppg_fetch.h) at every observation geometry the project supports, shared
by the wave-emulator tests (test_images_emulated.py) and the GPU tests (test_images_gpu.py).  No tests of its own.

The reference of every check is built here in plain numpy from `.cpu()` copies of the env tensors and the layout text of
include/ppg.h (section order, the 16-byte alignment rule, the record's field order): it uses none of the project's parsers.  Every
comparison is exact, section by section, observations as raw bits; padding bytes inside an image are unspecified and not compared.
Every output buffer is prefilled with 0xA5 and carries a 256-byte guard band behind the capacity the call is given.

Both kernels pick a copy loop at run time from the alignment of source, destination and length.  `pack_arms` / `fetch_arms` say,
from the reference tables alone, which loop every copy of an image takes; `assert_reach` holds every geometry to the arms it is
here for, so a seed or config change that silently stops reaching one fails on both backends.

A backend is a `Backend(make, make_rq, sync)`: `make(cfg, B, **kw)` builds a BatchedPredPreyGrass, `make_rq(cfg, B, **kw)` a
BatchedRedQueen.  One handle of 130 envs per geometry is stepped (`source`); the smaller handles of a handle set are handles of their
own batch size whose tensors are filled with a run of the source's envs (`clone`): the two kernels read nothing but those tensors."""
import collections
import ctypes as C
import struct

import numpy as np
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.config import config_env
from predpreygrass_amd.red_queen import config_env_base
from tests import pred_capacity_random as rand

Backend = collections.namedtuple("Backend", "make make_rq sync")

FILL, GUARD = 0xA5, 256
B_SOURCE = 130
F32, NO_OBS = 0x1, 0x2                         # include/ppg.h: PPG_PACK_F32, PPG_PACK_NO_OBS
PACK_MAGIC, FETCH_MAGIC = 0x4B475050, 0x46475050
EINVAL = -1
FLAG_SETS = (0, NO_OBS, NO_OBS | F32, F32)
# batch sizes of the handles of one ppg_pack call
HANDLE_SETS = {"1": (1,), "5": (5,), "1-64-2": (1, 64, 2), "65": (65,), "130": (130,), "1..8": (1, 2, 3, 4, 5, 6, 7, 8)}
FETCH_RANGES = ((0, 1), (129, 1), (3, 64), (1, 65), (0, 130))
FETCH_GEOMETRIES = ("a", "c", "e", "h", "i")

_DTYPES = {"float64": torch.float64, "float32": torch.float32, "bfloat16": torch.bfloat16}
# cheap births and predators that starve: row counts that differ from env to env within 25 calls
_BASE = {**config_env, "max_steps": 18, "predator_creation_energy_threshold": 6.0, "prey_creation_energy_threshold": 4.0,
         "energy_gain_per_step_grass": 0.2, "initial_energy_predator": 3.0, "initial_num_grass": 30}
_RQ = {**config_env_base, "max_steps": 18, "predator_creation_energy_threshold": 7.0, "prey_creation_energy_threshold": 4.0,
       "reproduction_cooldown_steps": 2, "n_initial_active_type_2_predator": 4, "n_possible_type_2_predators": 500,
       "initial_energy_predator": 3.0, "energy_loss_per_step_predator": 0.12, "initial_num_grass": 30}
_WALLS = [(4, y) for y in range(2, 7)] + [(x, 9) for x in range(6, 10)]

Geometry = collections.namedtuple("Geometry", "family dtype Rp Rq channels caps grid calls seed extra")
#   family: base | gen2 | walls (second generation + walls + visibility channel);  channels / caps: (predator, prey)
GEOMETRIES = {
    "a": Geometry("base", "float64", 7, 9, (4, 4), (64, 128), 12, 8, 1, {}),
    "b": Geometry("base", "float32", 3, 5, (4, 4), (64, 64), 10, 8, 2, {}),
    "c": Geometry("base", "bfloat16", 3, 5, (4, 4), (64, 128), 10, 8, 3, {}),
    "d": Geometry("base", "bfloat16", 1, 1, (4, 4), (64, 64), 8, 8, 4, {"initial_num_grass": 15}),
    "e": Geometry("walls", "float32", 3, 5, (5, 5), (64, 128), 12, 8, 5, {}),      # 144 cells: 5 wall words (odd)
    "f": Geometry("walls", "float64", 3, 5, (5, 5), (64, 128), 14, 8, 6, {}),      # 196 cells: 7 wall words
    "g": Geometry("base", "float64", 5, 7, (5, 7), (64, 128), 12, 8, 7,
                  {"enable_drive_channels": True, "predator_drive_channels": ["hunger_pressure"],
                   "prey_drive_channels": ["hunger_pressure", "reproductive_readiness", "grass_opportunity"]}),
    "h": Geometry("gen2", "float32", 7, 9, (4, 4), (64, 128), 14, 8, 8, {}),
    # 70 predators and 140 prey from the reset on: rows in use beyond the first trip of the kernels' `r += 64` loops
    "i": Geometry("base", "float32", 3, 3, (4, 4), (128, 256), 16, 2, 9,
                  {"n_initial_active_predator": 70, "n_initial_active_prey": 150, "initial_num_grass": 20, "max_steps": 30}),
    "j": Geometry("base", "float64", 15, 15, (4, 4), (64, 64), 16, 8, 10, {}),
}


def _geom(g):
    """A geometry by id, or the Geometry itself (the cases outside the table)."""
    return GEOMETRIES[g] if isinstance(g, str) else g


def geometry_config(gid):
    g = _geom(gid)
    cfg = dict(_BASE if g.family == "base" else _RQ)
    cfg.update(grid_size=g.grid, predator_obs_range=g.Rp, prey_obs_range=g.Rq)
    if g.family == "walls":
        cfg["include_visibility_channel"] = True
    cfg.update(g.extra)
    return cfg


def elem_bytes(g):
    return {"float64": 8, "float32": 4, "bfloat16": 2}[g.dtype]


def blocks(g):
    """Elements of one observation block: channels * R * R."""
    return g.channels[0] * g.Rp * g.Rp, g.channels[1] * g.Rq * g.Rq


def new_handle(bk, gid, B, seed=0):
    g = _geom(gid)
    kw = dict(obs_dtype=_DTYPES[g.dtype], pred_capacity=g.caps[0], prey_capacity=g.caps[1], seed=seed)
    if g.family == "base":
        env = bk.make(geometry_config(gid), B, **kw)
    else:
        env = bk.make_rq(geometry_config(gid), B, walls=g.family == "walls", **kw)
    assert (env.pred_capacity, env.prey_capacity) == g.caps and env.obs_pred.dtype == _DTYPES[g.dtype]
    assert tuple(env.obs_pred.shape[2:]) == (g.channels[0], g.Rp, g.Rp) and tuple(env.obs_prey.shape[2:]) == (g.channels[1], g.Rq, g.Rq)
    # (pack_arms / fetch_arms take the env tensors as 16-byte aligned)
    assert env.obs_pred.data_ptr() % 16 == 0 and env.obs_prey.data_ptr() % 16 == 0
    return env


def source(bk, gid, B=B_SOURCE):
    """The stepped handle of a geometry: reset and at most 25 calls with device random actions and auto-reset."""
    g = GEOMETRIES[gid]
    assert 8 <= g.grid <= 16 and g.calls <= 25
    if gid == "i":
        env = rand.env_with_many_predators(lambda cfg, _b, **kw: new_handle(bk, gid, B, seed=kw["seed"]), None, g.calls, seed=g.seed)
    else:
        env = new_handle(bk, gid, B, seed=g.seed)
        if g.family == "walls":
            env.set_walls(_WALLS)
        env.reset()
        for _ in range(g.calls):
            env.step(random_actions=True, auto_reset=True)
    bk.sync()
    return env


def clone(bk, gid, src, lo, n):
    """A handle of n envs whose tensors hold envs [lo, lo + n) of `src`."""
    env = new_handle(bk, gid, n)
    for name in _abi._BUF_FIELDS:
        getattr(env, name).copy_(getattr(src, name)[lo:lo + n])
    bk.sync()
    return env


class HandleFactory:
    """The handles of the handle sets of one geometry, built once each from runs of the source's envs."""

    def __init__(self, bk, gid, src):
        self.bk, self.gid, self.src, self._made = bk, gid, src, {}

    def handles(self, batches):
        total = sum(batches)
        lo = 0 if len(batches) > 1 else self.src.batch_size - total   # (single small handles: the source's LAST envs)
        out = []
        for n in batches:
            if n == self.src.batch_size:
                out.append(self.src)
            else:
                if (lo, n) not in self._made:
                    self._made[(lo, n)] = clone(self.bk, self.gid, self.src, lo, n)
                out.append(self._made[(lo, n)])
            lo += n
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# host copies of the env tensors
# ---------------------------------------------------------------------------------------------------------------------------------

_TABLES = ("row_xy", "row_energy", "row_id", "row_key", "row_cumrew", "row_flags", "row_reward", "row_parent", "env_state", "env_seed",
           "grass_xy", "grass_energy", "row_lastrep", "row_info", "wall_bits")
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _obs_bits(t):
    """[B, rows, block] unsigned integers holding the bits of an observation tensor."""
    t = t.cpu()
    size = t.element_size()
    return t.view(_BITS[size]).numpy().view(f"<u{size}").reshape(t.shape[0], t.shape[1], -1).copy()


def host_state(env):
    s = {n: getattr(env, n).cpu().numpy().copy() for n in _TABLES}
    s["obs_pred"], s["obs_prey"] = _obs_bits(env.obs_pred), _obs_bits(env.obs_prey)
    if env.obs_pred.dtype == torch.float64:   # (the values, for PPG_PACK_F32)
        s["val_pred"] = env.obs_pred.cpu().numpy().reshape(s["obs_pred"].shape).copy()
        s["val_prey"] = env.obs_prey.cpu().numpy().reshape(s["obs_prey"].shape).copy()
    s["cp"], s["S"] = env.pred_capacity, env.S
    return s


def align16(v):
    return (v + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------------------------------------
# ppg_pack: the reference image
# ---------------------------------------------------------------------------------------------------------------------------------

PACK_SECTIONS = ("env_state", "row_off", "id_pred", "id_prey", "reward_pred", "reward_prey", "flags_pred", "flags_prey", "obs_pred",
                 "obs_prey")
PackRef = collections.namedtuple("PackRef", "header offsets sections total n_rows row_off blk src_elem dst_elem")


def _in_use(states, name, species):
    """The rows in use of one table, env-major, handles in order: the FIRST env_state[PPG_ENV_N_*_ROWS] rows of the species."""
    word = _abi.ENV_N_PREY_ROWS if species else _abi.ENV_N_PRED_ROWS
    out = []
    for s in states:
        lo = s["cp"] if (species and name.startswith("row_")) else 0
        for b in range(len(s["env_state"])):
            out.append(s[name][b, lo:lo + int(s["env_state"][b, word])])
    return np.concatenate(out)


def pack_reference(states, gid, flags):
    """include/ppg.h: ppg_pack_header | env_state | row_off | id_pred | id_prey | reward_pred | reward_prey | flags_pred | flags_prey |
    obs_pred | obs_prey, every section 16-byte aligned."""
    g = _geom(gid)
    src = elem_bytes(g)
    dst = 4 if (flags & F32 and src == 8) else src
    blk = (0, 0) if flags & NO_OBS else blocks(g)
    es = np.concatenate([s["env_state"] for s in states]).astype("<i4")
    n = len(es)
    counts = np.stack([es[:, _abi.ENV_N_PRED_ROWS], es[:, _abi.ENV_N_PREY_ROWS]], axis=1).astype(np.int64)
    row_off = (np.cumsum(counts, axis=0) - counts).astype("<u4")
    n_rows = counts.sum(axis=0)
    sec = {"env_state": es, "row_off": row_off}
    for sp, tag in enumerate(("pred", "prey")):
        sec[f"id_{tag}"] = _in_use(states, "row_id", sp).astype("<i4")
        sec[f"reward_{tag}"] = _in_use(states, "row_reward", sp).astype("<f8")
        sec[f"flags_{tag}"] = _in_use(states, "row_flags", sp).astype("u1")
        if flags & NO_OBS:
            sec[f"obs_{tag}"] = np.zeros(0, np.uint8)
        elif dst != src:   # float64 rows travel as float32: round to nearest even, like the kernel's cast
            sec[f"obs_{tag}"] = _in_use(states, f"val_{tag}", sp).astype(np.float32).view("<u4")
        else:
            sec[f"obs_{tag}"] = _in_use(states, f"obs_{tag}", sp)
        assert sec[f"obs_{tag}"].size == int(n_rows[sp]) * blk[sp]
    offsets, o = {}, 64
    sections = {}
    for name in PACK_SECTIONS:
        raw = np.frombuffer(np.ascontiguousarray(sec[name]).tobytes(), np.uint8)
        offsets[name], sections[name] = o, raw
        o = align16(o + raw.size)
    header = dict(magic=PACK_MAGIC, version=1, n_envs=n, n_pred_rows=int(n_rows[0]), n_prey_rows=int(n_rows[1]), obs_elem_bytes=dst,
                  blk_pred=blk[0], blk_prey=blk[1], bytes_used=o, overflow=0, env_words=_abi.ENV_WORDS, reserved0=0, reserved1=0)
    return PackRef(header, offsets, sections, o, n_rows, row_off, blk, src, dst)


_PACK_HEADER = ("magic", "version", "n_envs", "n_pred_rows", "n_prey_rows", "obs_elem_bytes", "blk_pred", "blk_prey", "bytes_used",
                "capacity", "overflow", "env_words", "reserved0", "reserved1")


def pack_header(img):
    return dict(zip(_PACK_HEADER, struct.unpack("<8I2Q4I", img[:64].tobytes())))


def _same(img, off, want, tag):
    got = img[off:off + want.size]
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{tag}: first difference at byte {at} of the section (image offset {off + at}), "
                             f"got {got[at:at + 8].tolist()} want {want[at:at + 8].tolist()}")


def run_pack(bk, envs, flags, capacity, size, shift=0):
    """ppg_pack into a buffer of `size` bytes prefilled with 0xA5 -> (return code, the buffer on the host)."""
    e0 = envs[0]
    buf = torch.full((size,), FILL, dtype=torch.uint8, device=e0.device)
    assert buf.data_ptr() % 16 == 0
    handles = (C.c_void_p * len(envs))(*[e._handle for e in envs])
    rc = e0._lib.ppg_pack(handles, len(envs), C.c_void_p(buf.data_ptr() + shift), int(capacity), int(flags), e0._stream())
    bk.sync()
    return rc, buf.cpu().numpy()


def check_pack(bk, envs, gid, flags, tag, states=None):
    """One image with room to spare: return code, every header field, bytes_used == the reference's total == ppg_pack_bytes, every
    section, and the guard band.  Returns the reference."""
    states = states if states is not None else [host_state(e) for e in envs]
    ref = pack_reference(states, gid, flags)
    e0, need = envs[0], ref.total
    assert need == int(e0._lib.ppg_pack_bytes(e0._handle, ref.header["n_envs"], int(ref.n_rows[0]), int(ref.n_rows[1]), flags)), (tag, "ppg_pack_bytes")
    rc, img = run_pack(bk, envs, flags, need + GUARD, need + GUARD)
    assert rc == 0, (tag, rc, e0._lib.ppg_last_error(e0._handle))
    assert pack_header(img) == dict(ref.header, capacity=need + GUARD), (tag, pack_header(img), ref.header)
    for name in PACK_SECTIONS:
        _same(img, ref.offsets[name], ref.sections[name], f"{tag} {name}")
    assert (img[need:] == FILL).all(), (tag, "bytes behind bytes_used were written")
    return ref


def check_pack_capacity_edges(bk, envs, gid, flags, tag, states=None):
    """capacity == need: complete, no overflow.  capacity == need - 16: overflow = 1, bytes_used = need, env words and row_off right,
    nothing from the id_pred offset on is touched."""
    states = states if states is not None else [host_state(e) for e in envs]
    ref = pack_reference(states, gid, flags)
    need = ref.total
    rc, img = run_pack(bk, envs, flags, need, need + GUARD)
    assert rc == 0 and pack_header(img) == dict(ref.header, capacity=need), (tag, rc, pack_header(img))
    for name in PACK_SECTIONS:
        _same(img, ref.offsets[name], ref.sections[name], f"{tag} exact fit, {name}")
    assert (img[need:] == FILL).all(), (tag, "exact fit: the guard band was written")
    rc, img = run_pack(bk, envs, flags, need - 16, need + GUARD)
    assert rc == 0 and pack_header(img) == dict(ref.header, capacity=need - 16, overflow=1), (tag, rc, pack_header(img))
    for name in ("env_state", "row_off"):
        _same(img, ref.offsets[name], ref.sections[name], f"{tag} 16 bytes short, {name}")
    assert (img[ref.offsets["id_pred"]:] == FILL).all(), (tag, "16 bytes short: a row section was written")


def check_parse_image(envs, gid, flags, img, ref):
    """predpreygrass_amd.distributed.parse_image against the reference (observations as bits)."""
    from predpreygrass_amd.distributed import parse_image
    got = parse_image(torch.from_numpy(img))
    assert got["header"].bytes_used == ref.total and got["header"].obs_elem_bytes == ref.dst_elem
    for name in PACK_SECTIONS:
        t = got[name]
        if name.startswith("obs_"):
            assert t.element_size() == ref.dst_elem
        raw = t.contiguous().view(torch.uint8).numpy().reshape(-1)
        assert np.array_equal(raw, ref.sections[name]), (gid, flags, name)
    assert tuple(got["obs_pred"].shape) == (int(ref.n_rows[0]), ref.blk[0]) and tuple(got["obs_prey"].shape) == (int(ref.n_rows[1]), ref.blk[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# which copy loop every copy takes, from the reference tables alone
# ---------------------------------------------------------------------------------------------------------------------------------

def _pack16_trips(n16):
    """The 16-byte loops of pack_copy_obs / fetch_copy over n16 words: which of main loop (four words in flight per lane), tail and
    idle lanes occur."""
    out = set()
    for ln in range(64):
        i = ln
        while i + 192 < n16:
            out.add("16B main")
            i += 256
        if i < n16:
            out.add("16B tail")
    if 0 < n16 < 64:
        out.add("16B short")
    return out


def pack_arms(ref, species):
    """The arms of pack_copy_obs the envs of an image take for one species.  The source of an env's run starts a multiple of
    capacity * block bytes into a 16-byte aligned tensor, so it is 16-byte aligned; the destination is the 16-byte aligned section
    plus row_off * block bytes."""
    blk, arms = ref.blk[species], set()
    counts = np.diff(np.append(ref.row_off[:, species].astype(np.int64), ref.n_rows[species]))
    assert (64 * blk * ref.src_elem) % 16 == 0
    for n, off in zip(counts.tolist(), ref.row_off[:, species].tolist()):
        if n == 0 or blk == 0:
            continue
        n_elems, dst = n * blk, off * blk * ref.dst_elem
        if ref.src_elem == ref.dst_elem:
            nbytes = n_elems * ref.src_elem
            if (dst | nbytes) & 15 == 0:
                arms |= _pack16_trips(nbytes >> 4)
            else:
                arms.add({8: "double", 4: "float", 2: "uint16"}[ref.src_elem])
        elif (dst & 7) | (n_elems & 1) == 0:
            arms.add("f64->f32 pairs")
            if (n_elems >> 1) > 192:
                arms.add("f64->f32 pairs main")
        else:
            arms.add("f64->f32 scalar")
    return arms


def fetch_copy_arm(src, dst, n):
    return "16B" if (src | dst | n) & 15 == 0 else "4B" if (src | dst | n) & 3 == 0 else "1B"


# the arms of pack_copy_obs a geometry is here for: {flags: arms that BOTH species must reach}
REACH = {
    "a": {0: {"16B main", "16B tail"}, F32: {"f64->f32 pairs", "f64->f32 pairs main"}},
    "b": {0: {"16B tail"}},   # (and "16B short" in the predator runs: assert_reach)
    "c": {0: {"uint16"}},
    "d": {0: {"uint16"}},
    "e": {0: {"float"}},
    "f": {0: {"double"}, F32: {"f64->f32 scalar"}},
    "g": {0: {"double"}, F32: {"f64->f32 scalar", "f64->f32 pairs"}},
    "h": {0: {"16B main"}},
    "i": {0: {"16B main"}},
    "j": {0: {"16B main", "16B tail"}},
}


def assert_reach(gid, refs):
    """refs: {flags: PackRef of the 130-env image}.  The geometry reaches what it is in the table for."""
    g, ref = GEOMETRIES[gid], refs[0]
    counts = np.stack([np.diff(np.append(ref.row_off[:, sp].astype(np.int64), ref.n_rows[sp])) for sp in (0, 1)], axis=1)
    reached = {}
    for flags, want in REACH[gid].items():
        for sp in (0, 1):
            reached[(flags, sp)] = pack_arms(refs[flags], sp)
            assert want <= reached[(flags, sp)], (gid, flags, ("predators", "prey")[sp], sorted(reached[(flags, sp)]))
    run_bytes = counts * np.array(blocks(g)) * elem_bytes(g)
    if gid in "cefg":   # the unaligned arms need both: an env that starts at an odd row offset and an env with an odd row count
        for sp in (0, 1):
            assert (ref.row_off[:, sp] & 1).any() and (counts[:, sp] & 1).any(), (gid, sp)
    if gid == "a":
        assert run_bytes.max() > 8192
    if gid == "b":   # runs of fewer than 64 16-byte words: lanes without work
        assert ((run_bytes > 0) & (run_bytes < 64 * 16)).any() and "16B short" in reached[(0, 0)]
    if gid == "d":
        assert blocks(g)[0] * elem_bytes(g) == 8 and blocks(g)[1] * elem_bytes(g) == 8
    if gid == "i":   # the second trip of the `r += 64` loops over the rows, and a third over the prey rows
        assert counts[:, 0].max() > 64 and counts[:, 1].max() > 128, counts.max(axis=0)
    if gid == "j":
        assert blocks(g)[0] * elem_bytes(g) == 7200
    return reached


# ---------------------------------------------------------------------------------------------------------------------------------
# ppg_pack: the matrix of one geometry, and the calls it must refuse
# ---------------------------------------------------------------------------------------------------------------------------------

def pack_matrix(bk, gid, src, handle_sets=HANDLE_SETS, parsers=True):
    """Every handle set x every flag set of one geometry, the capacity edges of every handle set, the reach conditions on the 130-env
    image and parse_image once per flag set.  Returns {(flags, species): arms reached}."""
    factory = HandleFactory(bk, gid, src)
    refs = {}
    for set_id, batches in handle_sets.items():
        envs = factory.handles(batches)
        assert [e.batch_size for e in envs] == list(batches)
        states = [host_state(e) for e in envs]
        for flags in FLAG_SETS:
            ref = check_pack(bk, envs, gid, flags, f"{gid} handles {set_id} flags {flags}", states)
            if set_id == "130":
                refs[flags] = ref
        check_pack_capacity_edges(bk, envs, gid, 0, f"{gid} handles {set_id}", states)
        if set_id == "1-64-2":
            check_pack_capacity_edges(bk, envs, gid, F32, f"{gid} handles {set_id} F32", states)
            if parsers:
                for flags in FLAG_SETS:
                    ref = pack_reference(states, gid, flags)
                    rc, img = run_pack(bk, envs, flags, ref.total + GUARD, ref.total + GUARD)
                    assert rc == 0
                    check_parse_image(envs, gid, flags, img, ref)
    elem = elem_bytes(GEOMETRIES[gid])
    assert refs[F32].header["obs_elem_bytes"] == (4 if elem == 8 else elem)   # float32 / bfloat16 rows are copied
    if elem != 8:
        assert all(np.array_equal(refs[F32].sections[n], refs[0].sections[n]) for n in PACK_SECTIONS)
    return assert_reach(gid, refs) if "130" in handle_sets else {}


def pack_refusals(bk):
    """Calls that return PPG_EINVAL, leave the buffer untouched and leave a message in ppg_last_error."""
    h = new_handle(bk, "c", 2)
    h.reset()
    bk.sync()
    lib = h._lib
    need = pack_reference([host_state(h)], "c", 0).total

    def refused(envs, flags, capacity, word, shift=0):
        rc, img = run_pack(bk, envs, flags, capacity, need + GUARD, shift=shift)
        msg = lib.ppg_last_error(envs[0]._handle).decode()
        assert rc == EINVAL and word in msg, (word, rc, msg)
        assert (img == FILL).all(), (word, "the buffer was written")

    refused([h] * 9, 0, need, "at most 8 handles")
    for change in (dict(Rq=3), dict(dtype="float32"), dict(caps=(64, 64))):   # another Rq / dtype / prey capacity
        h2 = new_handle(bk, GEOMETRIES["c"]._replace(**change), 1)
        h2.reset()
        refused([h, h2], 0, need, "another geometry")
    refused([h], 0, need, "16-byte aligned", shift=8)
    refused([h], 0x4, need, "unknown pack flags")
    fixed = align16(align16(64 + 2 * _abi.ENV_WORDS * 4) + 2 * 8)
    refused([h], 0, fixed - 16, "below the fixed part")
    rc, img = run_pack(bk, [h], NO_OBS, fixed, need + GUARD)   # (the fixed part itself is enough to be told the size)
    assert rc == 0 and pack_header(img)["overflow"] == 1


_CFG_STARVE = {**config_env, "grid_size": 10, "n_initial_active_predator": 1, "energy_loss_per_step_predator": 2.0,
               "initial_num_grass": 20}


def pack_env_without_predators(bk):
    """One predator that starves, no auto-reset: an env whose PPG_ENV_N_PRED_ROWS is 0, packed in front of envs that have rows (their
    offsets must not move).  Returns the number of calls it took."""
    env = bk.make(_CFG_STARVE, 5, seed=1)
    env.reset()
    for call in range(1, 51):
        env.step(random_actions=True)
        bk.sync()
        if int(env.env_state[:, _abi.ENV_N_PRED_ROWS].min()) == 0:
            break
    else:
        raise AssertionError("no env lost all its predator rows within 50 calls")
    full = bk.make(_CFG_STARVE, 3, seed=7)
    full.reset()
    full.step(random_actions=True)
    bk.sync()
    assert int(full.env_state[:, _abi.ENV_N_PRED_ROWS].min()) > 0
    g = Geometry("base", "float64", 7, 9, (4, 4), (64, 128), 10, call, 1, {})
    for envs in ([env], [env, full], [full, env, full]):
        for flags in FLAG_SETS:
            ref = check_pack(bk, envs, g, flags, f"no predator rows, {len(envs)} handles, flags {flags}")
        assert (np.diff(np.append(ref.row_off[:, 0].astype(np.int64), ref.n_rows[0])) == 0).any()
        check_pack_capacity_edges(bk, envs, g, 0, "no predator rows")
    return call


# ---------------------------------------------------------------------------------------------------------------------------------
# ppg_fetch: the reference image
# ---------------------------------------------------------------------------------------------------------------------------------

FetchRef = collections.namedtuple("FetchRef", "header record_bytes fields records sections fixed used n_rows")


def record_fields(gid, S, NG, n_wall_words):
    """include/ppg.h: (name, bytes) of an env's record in order; each slice is padded to 8 bytes, the record to 16."""
    g = GEOMETRIES[gid]
    f = [("row_xy", 2 * S), ("row_energy", 8 * S), ("row_id", 4 * S), ("row_key", 4 * S), ("row_cumrew", 8 * S), ("row_flags", S),
         ("row_reward", 8 * S), ("row_parent", 4 * S), ("env_state", 4 * _abi.ENV_WORDS), ("env_seed", 8), ("grass_xy", 2 * NG),
         ("grass_energy", 8 * NG)]
    if g.family != "base":
        f.append(("row_lastrep", 4 * S))
    if g.family == "walls":
        f += [("row_info", S), ("wall_bits", 4 * n_wall_words)]
    return f


def fetch_reference(state, gid, env0, n):
    g = GEOMETRIES[gid]
    S, NG, W = state["S"], state["grass_xy"].shape[1], state["wall_bits"].shape[1]
    assert W == (g.grid * g.grid + 31) // 32
    fields, off = [], 0
    for name, nbytes in record_fields(gid, S, NG, W):
        assert state[name][0].nbytes == nbytes, (name, state[name][0].nbytes, nbytes)
        fields.append((name, off, nbytes))
        off += (nbytes + 7) // 8 * 8
    rec = align16(off)
    bp, bq = blocks(g)[0] * elem_bytes(g), blocks(g)[1] * elem_bytes(g)
    records = [{name: np.frombuffer(state[name][env0 + i].tobytes(), np.uint8) for name, _, _ in fields} for i in range(n)]
    fixed = 64 + n * rec
    sections, o, n_rows = [], fixed, [0, 0]
    for i in range(n):
        es = state["env_state"][env0 + i]
        for sp, (tag, word) in enumerate((("obs_pred", _abi.ENV_N_PRED_ROWS), ("obs_prey", _abi.ENV_N_PREY_ROWS))):
            raw = np.frombuffer(state[tag][env0 + i, :int(es[word])].tobytes(), np.uint8)
            assert raw.size == int(es[word]) * (bp, bq)[sp]
            sections.append((i, tag, o, raw))
            o += align16(raw.size)
            n_rows[sp] += int(es[word])
    header = dict(magic=FETCH_MAGIC, version=1, env0=env0, n_envs=n, record_bytes=rec, blk_pred_bytes=bp, blk_prey_bytes=bq, overflow=0,
                  bytes_used=o, reserved=(0, 0, 0, 0))
    return FetchRef(header, rec, fields, records, sections, fixed, o, n_rows)


def fetch_header(img):
    v = struct.unpack("<8I2Q4I", img[:64].tobytes())
    names = ("magic", "version", "env0", "n_envs", "record_bytes", "blk_pred_bytes", "blk_prey_bytes", "overflow", "bytes_used", "capacity")
    return dict(zip(names, v[:10]), reserved=tuple(v[10:]))


def fetch_arms(ref, state, env0):
    """The arms of fetch_copy an image takes: {"fields": ..., "obs": ...}.  Records and sections start 16-byte aligned in the image;
    an env's slice of a state tensor starts env * bytes into a 16-byte aligned tensor."""
    arms = {"fields": set(), "obs": set()}
    for i in range(ref.header["n_envs"]):
        for name, off, nbytes in ref.fields:
            arms["fields"].add(fetch_copy_arm((env0 + i) * nbytes, off, nbytes))
    for i, tag, o, raw in ref.sections:
        if raw.size:
            arms["obs"].add(fetch_copy_arm(0, 0, raw.size))
    return arms


def run_fetch(env, env0, n, capacity, size=None, shift=0):
    """ppg_fetch (the C entry) into a host buffer prefilled with 0xA5 -> (return code, a copy of the buffer)."""
    host = env._host_buffer((int(capacity) if size is None else size) + GUARD)
    host.fill_(FILL)
    assert host.data_ptr() % 16 == 0
    rc = env._lib.ppg_fetch(env._handle, int(env0), int(n), C.c_void_p(host.data_ptr() + shift), int(capacity), env._stream())
    return rc, host.numpy().copy()


def check_fetch(env, gid, state, env0, n, tag, capacity=None):
    """One range: header, every field of every record, every observation section, the guard band.  capacity=None: the upper bound
    ppg_fetch_bytes gives for the range's row totals."""
    ref = fetch_reference(state, gid, env0, n)
    bound = int(env._lib.ppg_fetch_bytes(env._handle, n, ref.n_rows[0], ref.n_rows[1]))
    assert ref.used <= bound, (tag, ref.used, bound)
    capacity = bound if capacity is None else capacity
    rc, img = run_fetch(env, env0, n, capacity)
    assert rc == 0, (tag, rc, env._lib.ppg_last_error(env._handle))
    overflow = int(ref.used > capacity)
    assert fetch_header(img) == dict(ref.header, capacity=capacity, overflow=overflow), (tag, fetch_header(img), ref.header)
    for i, record in enumerate(ref.records):
        for name, off, nbytes in ref.fields:
            _same(img, 64 + i * ref.record_bytes + off, record[name], f"{tag} env {env0 + i} {name}")
    if not overflow:
        for i, name, o, raw in ref.sections:
            _same(img, o, raw, f"{tag} env {env0 + i} {name}")
    assert (img[capacity:] == FILL).all(), (tag, "bytes at or behind the capacity were written")
    return ref


def fresh_copy(bk, gid, src):
    """A handle that has never been fetched from, holding the source's state."""
    return clone(bk, gid, src, 0, src.batch_size)


def fetch_matrix(bk, gid, src):
    """The ranges, the small-large-small sequence on a fresh handle, the overflowing capacity, the refused calls and (float64 /
    float32) the Python fetch() of one geometry.  Returns the arms reached."""
    g = GEOMETRIES[gid]
    B = src.batch_size
    assert B == B_SOURCE
    state = host_state(src)
    arms = {"fields": set(), "obs": set()}
    for env0, n in FETCH_RANGES:
        ref = check_fetch(src, gid, state, env0, n, f"{gid} fetch({env0}, {n})")
        got = fetch_arms(ref, state, env0)
        arms = {k: arms[k] | got[k] for k in arms}
    # a fresh handle: (0, 1) sizes the staging buffer and the first transfer for ONE env; (0, 130) then has to regrow the buffer and
    # to bring the observation sections in a second transfer; (0, 1) again runs in the larger buffer with the larger hint
    fresh = fresh_copy(bk, gid, src)
    small = check_fetch(fresh, gid, state, 0, 1, f"{gid} fresh handle, fetch(0, 1)")
    large = fetch_reference(state, gid, 0, B)
    hint = small.used + small.used // 4 + 4096   # (ppg_learner_host.h: what the next call copies in its first transfer, at least the fixed part)
    assert large.used > max(hint, large.fixed), "the large image must not fit the first transfer"
    check_fetch(fresh, gid, state, 0, B, f"{gid} fresh handle, fetch(0, {B}) after fetch(0, 1)")
    check_fetch(fresh, gid, state, 0, 1, f"{gid} fresh handle, fetch(0, 1) again")
    # header + records + 16 bytes: overflow, the size it needs, valid records
    for env0, n in ((0, B), (3, 64)):
        ref = fetch_reference(state, gid, env0, n)
        assert ref.used > ref.fixed + 16
        check_fetch(src, gid, state, env0, n, f"{gid} fetch({env0}, {n}) into the fixed part + 16", capacity=ref.fixed + 16)
    one = fetch_reference(state, gid, 0, 1)
    for args, kw in (((0, 1, one.used), dict(shift=8, size=one.used + 16)), ((B - 1, 2, 2 * one.used + 65536), {}),
                     ((1, B, large.used + 65536), {}), ((0, 0, one.used), {}), ((0, 1, one.fixed - 16), dict(size=one.used)),
                     ((0, 2, one.fixed), dict(size=one.used))):
        rc, img = run_fetch(src, *args, **kw)
        assert rc == EINVAL and (img == FILL).all(), (gid, args, rc)
    if g.dtype != "bfloat16":
        for env0, n in ((0, 1), (3, 64), (0, B)):
            check_python_fetch(src, gid, state, env0, n)
    if gid == "c":   # an odd number of 72-byte blocks
        assert "4B" in arms["obs"]
    if gid == "e":   # env_seed (8 bytes) and five wall words
        assert "4B" in arms["fields"] and dict((n, b) for n, _, b in ref.fields)["wall_bits"] % 8 == 4
    if gid == "i":
        counts = state["env_state"][:, [_abi.ENV_N_PRED_ROWS, _abi.ENV_N_PREY_ROWS]]
        assert counts[:, 0].max() > 64 and counts[:, 1].max() > 128
    assert "16B" in arms["obs"] | arms["fields"]
    # no supported geometry reaches the byte loop: every field is a multiple of 4 bytes, every observation block of 8
    assert "1B" not in arms["obs"] | arms["fields"]
    return arms


def check_python_fetch(env, gid, state, env0, n):
    """BatchedPredPreyGrass.fetch against the reference."""
    ref = fetch_reference(state, gid, env0, n)
    tables, obs_p, obs_q = env.fetch(env0, n)
    for name, _, _ in ref.fields:
        for i in range(n):
            assert np.array_equal(np.frombuffer(np.ascontiguousarray(tables[name][i]).tobytes(), np.uint8), ref.records[i][name]), (gid, name, env0 + i)
    got = {"obs_pred": obs_p, "obs_prey": obs_q}
    for i, tag, _, raw in ref.sections:
        a = np.ascontiguousarray(got[tag][i])
        assert a.shape[1:] == tuple(getattr(env, tag).shape[2:]) and a.dtype.itemsize == elem_bytes(GEOMETRIES[gid])
        assert np.array_equal(np.frombuffer(a.tobytes(), np.uint8), raw), (gid, tag, env0 + i)


def everything(bk, geometries=tuple(GEOMETRIES), handle_sets=HANDLE_SETS, step_bk=None):
    """The pack and the fetch matrix of the given geometries and the geometry-independent cases (the sanitizer leg runs this).
    step_bk: another backend that steps the source, whose state is then copied into a handle of `bk`."""
    for gid in geometries:
        src = source(step_bk or bk, gid)
        if step_bk is not None:
            src = clone(bk, gid, src, 0, src.batch_size)
        pack_matrix(bk, gid, src, handle_sets)
        if gid in FETCH_GEOMETRIES:
            fetch_matrix(bk, gid, src)
    pack_refusals(bk)
    pack_env_without_predators(bk)
