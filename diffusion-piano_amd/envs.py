"""Batched PianoWithShadowHands environments on the MI355X kernel.

Host-side mirror of the reference's interface for the hot path:

* :class:`VectorizedPianoEnv` - the VecEnv surface of ``parallelized_base_v2.py:21-67``
  (``reset() -> obs dict``, ``step(actions) -> (obs dict, rewards, dones)``,
  ``envs[i].observation_spec()/action_spec()``) plus the ``observation_spec`` /
  ``action_spec`` attributes of ``parallelized_base.py:87-89``.
* :class:`BatchedPianoEnv` - the torch-native core: flat ``[N, obs_dim]`` observations,
  rewards, discounts and dm_env step types as torch-ROCm tensors; no host round trip.
* :func:`load` - ``robopianist.suite.load`` (suite/__init__.py:50-93) for one env,
  returning dm_env ``TimeStep`` objects.

Task options follow ``PianoWithShadowHands.__init__`` (piano_with_shadow_hands.py:50-66).
Every compute call goes through libpianosim.so; there is no CPU fallback.
"""

from __future__ import annotations

import ctypes as C
import enum
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib, abi, model as model_lib, music, variations


# ---------------------------------------------------------------- dm_env (not installed)
class StepType(enum.IntEnum):
    FIRST = abi.FIRST
    MID = abi.MID
    LAST = abi.LAST

    def first(self) -> bool:
        return self is StepType.FIRST

    def mid(self) -> bool:
        return self is StepType.MID

    def last(self) -> bool:
        return self is StepType.LAST


class TimeStep(NamedTuple):
    """dm_env.TimeStep: FIRST carries reward/discount None."""

    step_type: Any
    reward: Any
    discount: Any
    observation: Any

    def first(self) -> bool:
        return self.step_type == StepType.FIRST

    def mid(self) -> bool:
        return self.step_type == StepType.MID

    def last(self) -> bool:
        return self.step_type == StepType.LAST


class Array(NamedTuple):
    shape: tuple
    dtype: Any
    name: str = ""


class BoundedArray(NamedTuple):
    shape: tuple
    dtype: Any
    minimum: np.ndarray
    maximum: np.ndarray
    name: str = ""


# ---------------------------------------------------------------- task configuration
class HandSide(str, enum.Enum):
    """``robopianist.models.hands.HandSide`` for ``TaskConfig.hand_side``; the plain strings
    "right" / "left" are accepted too."""

    RIGHT = "right"
    LEFT = "left"


@dataclass
class TaskConfig:
    """``PianoWithShadowHands`` keyword arguments (piano_with_shadow_hands.py:50-66) plus the
    solver settings of this implementation."""

    n_steps_lookahead: int = 1
    n_seconds_lookahead: Optional[float] = None
    trim_silence: bool = False
    wrong_press_termination: bool = False
    initial_buffer_time: float = 0.0
    disable_fingering_reward: bool = False
    disable_forearm_reward: bool = False
    disable_colorization: bool = False  # render()'s default for `colorize` (fingertip and goal-key colours)
    disable_hand_collisions: bool = False
    energy_penalty_coef: float = 5e-3
    randomize_hand_positions: bool = False  # piano_with_shadow_hands.py:64,491-499
    control_timestep: float = model_lib.CONTROL_TIMESTEP
    physics_timestep: float = model_lib.PHYSICS_TIMESTEP
    # Constraint solve: "newton" (alias "exact") = MuJoCo's primal problem minimised by Newton
    # iterations with exact line search (mj_solNewton), to convergence - the unique solution
    # every MuJoCo solver converges to. `solver_iterations` caps the Newton iterations per
    # substep (None: the library default, 24). The round-1 truncated "pgs" is retired.
    constraint_solver: str = "newton"
    solver_iterations: Optional[int] = None
    # 0: the solve ends when its line search ends in the Hessian's piece (the exact minimiser, to
    # the fp32 factor's error); 1 (the default since round 6): one more Newton step in that piece
    # on coupled-hand substeps - the fp32 parity target of 1e-4 over all env-steps of the coupled /
    # heavy-contact / Guren cases needs it, ~5% of the throughput; 2: on
    # every substep. Solves that end in the previous substep's guessed piece are not refined
    # (ps_task_cfg.solver_refine)
    solver_refine: int = 1
    max_contacts: int = 20
    hand_xml: Optional[str] = None  # a user hand MJCF (path or text, mjcf.load_hand); None = authored hand
    # PianoTask keyword arguments (tasks/base.py:96-107, forwarded by PianoWithShadowHands'
    # **kwargs, piano_with_shadow_hands.py:65):
    gravity_compensation: bool = False  # gravcomp 1 on every hand body (tasks/base.py:185-186)
    attachment_yaw: float = model_lib.ATTACHMENT_YAW  # degrees, hand roots about z (tasks/base.py:174-181)
    # Fingertip colliders (shadow_hand.py:95,144-152). None: the authored hand (capsules
    # everywhere, this implementation's default); True: Menagerie-style palm boxes with capsule
    # distal colliders; False (the reference's default): palm boxes with convex-hull (mesh)
    # distal colliders, the step kernel's hull instantiation. Exclusive with hand_xml.
    primitive_fingertip_collisions: Optional[bool] = None
    # THJ5, THJ1, LFJ5 and their actuators removed, THJ2 narrowed (shadow_hand.py:73-79,164-183):
    # action 39, joints_pos 23 per hand
    reduced_action_space: bool = False
    # the forearm slides kept: a subset of ("forearm_tx", "forearm_ty") (shadow_hand.py:270-311)
    forearm_dofs: Tuple[str, ...] = model_lib.FOREARM_DOFS
    # Per-episode MIDI augmentations (piano_with_shadow_hands.py:62,151-157): variations.MidiSelect /
    # MidiTemporalStretch / MidiPitchShift / MidiOctaveShift, at most one of each, applied in this
    # order to the initial song at the start of every episode of every env, on the device.
    augmentations: Optional[Sequence[Any]] = None
    # the per-env song tables of an augmented handle may take this many bytes (488 per env and
    # row: DESIGN.md section 11); more is an error at create
    augmentation_max_bytes: int = 8 << 30
    # PianoWithOneShadowHand (piano_with_one_shadow_hand.py): "right" / "left" (or a HandSide) keeps
    # that hand only - the other is detached from the model. Action 23 (20 reduced); observations
    # goal, fingering (5 wide), piano/state, piano/sustain_state, <rh|lh>_shadow_hand/joints_pos
    # and /position; rewards key_press, sustain, energy and (with fingering) fingering - no OT
    # term, no forearm term. None: PianoWithShadowHands.
    hand_side: Optional[str] = None
    # Observables of the reference's entities beyond the task's default ones, by the reference's
    # names (abi.OBSERVABLES): the piano's as "piano/joints_pos", "piano/activation",
    # "piano/sustain_activation"; the hands' bare - "joints_pos_cos_sin", "joints_vel",
    # "actuators_force", "actuators_velocity", "actuators_power", "fingertip_positions", "position" -
    # for both hands (the kept one with hand_side, whose row has "position" already). They are
    # appended to the row after its default part, in the fixed order of ps_task_cfg.observables
    # whatever the order here; obs_layout names their slices. "joints_torque" and "fingertip_force"
    # are not modelled and are refused. None: the default row.
    observables: Optional[Sequence[str]] = None

    def side(self) -> Optional[str]:
        """hand_side as None, "right" or "left"."""
        if self.hand_side is None:
            return None
        v = self.hand_side.value if isinstance(self.hand_side, HandSide) else self.hand_side
        if v not in ("right", "left"):
            raise ValueError(f"hand_side must be None, 'right' or 'left', got {self.hand_side!r}")
        return v

    def lookahead(self) -> int:
        if self.n_seconds_lookahead is not None:
            return int(math.ceil(self.n_seconds_lookahead / self.control_timestep))
        return self.n_steps_lookahead


def _to_sequence(midi) -> music.NoteSequence:
    if isinstance(midi, music.NoteSequence):
        return midi
    if isinstance(midi, (str, Path)):
        return music.parse_midi(midi)
    raise TypeError(f"unsupported midi input {type(midi)!r}")


def initial_sequence(midi, cfg: TaskConfig) -> music.NoteSequence:
    """The task's initial song: the constructor's midi, trimmed when ``trim_silence``
    (piano_with_shadow_hands.py:100-103)."""
    seq = _to_sequence(midi)
    return music.trim_silence(seq) if cfg.trim_silence else seq


def compile_task(midi, cfg: TaskConfig, canonical_actions: bool = True):
    """-> (ps_model_desc, SongTables, ps_task_cfg) for a song and task options."""
    if isinstance(midi, music.SongTables):
        song = midi
    else:
        song = music.song_tables(initial_sequence(midi, cfg), cfg.control_timestep, cfg.initial_buffer_time)
    hand = None
    side = cfg.side()
    if side is not None and cfg.randomize_hand_positions:
        raise ValueError("randomize_hand_positions is an option of the two-hand task: the one-hand task "
                         "(hand_side) has none")
    if cfg.hand_xml is not None and cfg.primitive_fingertip_collisions is not None:
        raise ValueError("hand_xml and primitive_fingertip_collisions are exclusive: the MJCF names its colliders")
    if isinstance(cfg.observables, str):
        raise TypeError("observables is a sequence of names, not one string")
    observables = abi.obs_mask(cfg.observables)  # (before the model is built: a bad name costs nothing)
    if cfg.hand_xml is not None:
        from . import mjcf
        hand = mjcf.load_hand(cfg.hand_xml)
    elif cfg.primitive_fingertip_collisions is not None:
        from . import mjcf
        hand = mjcf.box_hull_hand(hull_fingertips=not cfg.primitive_fingertip_collisions)
    md = model_lib.build_model(control_timestep=cfg.control_timestep,
                               physics_timestep=cfg.physics_timestep,
                               hand_collisions=not cfg.disable_hand_collisions, hand=hand,
                               gravity_compensation=cfg.gravity_compensation,
                               attachment_yaw=cfg.attachment_yaw,
                               reduced_action_space=cfg.reduced_action_space,
                               forearm_dofs=cfg.forearm_dofs, hand_side=side)
    tc = abi.TaskCfg()
    tc.hand_side = abi.HAND_BOTH if side is None else 1 + model_lib.HAND_SIDES[side]
    tc.n_steps_lookahead = cfg.lookahead()
    tc.fingering_reward = int(not cfg.disable_fingering_reward and song.has_fingering)
    tc.forearm_reward = int(not cfg.disable_forearm_reward)
    tc.wrong_press_termination = int(cfg.wrong_press_termination)
    tc.energy_penalty_coef = cfg.energy_penalty_coef
    if cfg.constraint_solver not in ("newton", "exact"):
        raise ValueError(f"constraint_solver must be 'newton' (or its alias 'exact'), got {cfg.constraint_solver!r}"
                         " (the round-1 truncated 'pgs' solver is retired)")
    tc.solver = abi.SOLVER_NEWTON
    tc.solver_iterations = 0 if cfg.solver_iterations is None else int(cfg.solver_iterations)
    if cfg.solver_refine not in (0, 1, 2):
        raise ValueError(f"solver_refine must be 0, 1 or 2, got {cfg.solver_refine!r}")
    tc.solver_refine = int(cfg.solver_refine)
    tc.randomize_hand_positions = int(cfg.randomize_hand_positions)
    tc.max_contacts = min(cfg.max_contacts, abi.MAX_CONTACTS_LIMIT)
    tc.canonical_actions = int(canonical_actions)
    tc.observables = observables
    return md, song, tc


def obs_layout(tc: abi.TaskCfg, md: Optional[abi.ModelDesc] = None) -> Dict[str, slice]:
    """Observation keys in the order the reference driver concatenates them
    (parallelized_base_v2.py:122-131); joints_pos as wide as the model's hands (``md``). The
    one-hand task (``tc.hand_side``): fingering 5 wide, the kept hand's joints_pos, then its root
    position (piano_with_one_shadow_hand.py:297-318, hands/base.py:112-114)."""
    out, o = {}, 0
    g = (tc.n_steps_lookahead + 1) * (abi.NKEY + 1)
    out["goal"] = slice(o, o + g); o += g
    nf = 5 if tc.hand_side else 10
    if tc.fingering_reward:
        out["fingering"] = slice(o, o + nf); o += nf
    out["piano/state"] = slice(o, o + abi.NKEY); o += abi.NKEY
    out["piano/sustain_state"] = slice(o, o + 1); o += 1
    nj = abi.obs_joints(md)
    if tc.hand_side:
        h = tc.hand_side - 1
        name = ("rh", "lh")[h] + "_shadow_hand"
        out[name + "/joints_pos"] = slice(o, o + nj[h]); o += nj[h]
        out[name + "/position"] = slice(o, o + 3); o += 3
    else:
        out["rh_shadow_hand/joints_pos"] = slice(o, o + nj[0]); o += nj[0]
        out["lh_shadow_hand/joints_pos"] = slice(o, o + nj[1]); o += nj[1]
    # the extras of tc.observables follow the default part, in their fixed order
    for key, w in abi.obs_extras(tc, md):
        out[key] = slice(o, o + w); o += w
    return out


# ---------------------------------------------------------------- batched core
class BatchedPianoEnv:
    """N envs on one GPU; all tensors live in HBM (torch-ROCm)."""

    def __init__(self, num_envs: int, midi, task: Optional[TaskConfig] = None, device=None,
                 canonical_actions: bool = True, seed: int = 0, env_offset: int = 0, _compiled=None):
        """``seed`` keys the per-env random draws (randomize_hand_positions); ``env_offset`` is the
        global id of env 0 when one job's envs are sharded over GPUs (sharding.EnvShard.start), so
        global env g draws the same values at any world size."""
        import torch

        self._torch = torch
        if not torch.cuda.is_available():
            raise _lib.PianosimError("BatchedPianoEnv needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.task = task or TaskConfig()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.num_envs = int(num_envs)
        if _compiled is not None:  # from_compiled: the caller's descriptors as they are
            self.model_desc, self.song, self.task_cfg = _compiled
            canonical_actions = bool(self.task_cfg.canonical_actions)
        else:
            self.model_desc, self.song, self.task_cfg = compile_task(midi, self.task, canonical_actions)
        self.canonical_actions = canonical_actions
        self.obs_dim = abi.obs_dim(self.task_cfg, self.model_desc)
        self.obs_slices = obs_layout(self.task_cfg, self.model_desc)
        self.action_dim = model_lib.action_dim(self.model_desc)
        self.action_lo, self.action_hi = model_lib.action_spec(self.model_desc)
        L = _lib.load()
        sd = abi.SongDesc.from_tables(self.song)
        if L.ps_model_desc_size() != C.sizeof(abi.ModelDesc):
            raise _lib.PianosimError("ps_model_desc layout mismatch between abi.py and the library")
        h = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(L.ps_create(C.addressof(self.model_desc), C.addressof(sd), C.addressof(self.task_cfg),
                               self.num_envs, dev_index, seed, C.byref(h)))
        self._h = h
        if hasattr(L, "ps_env_obs_dim") and (L.ps_env_obs_dim(h) != self.obs_dim or
                                             L.ps_env_action_dim(h) != self.action_dim):
            raise _lib.PianosimError("observation / action layout mismatch between the host and the library")
        if env_offset:
            _lib.check(L.ps_set_env_offset(h, int(env_offset)))
        self.augmentations = None
        if self.task.augmentations is not None:
            self._set_augmentations(midi)
        N = self.num_envs
        f32 = dict(device=self.device, dtype=torch.float32)
        self.obs = torch.zeros(N, self.obs_dim, **f32)
        self.reward = torch.zeros(N, **f32)
        self.discount = torch.ones(N, **f32)
        self.step_type = torch.zeros(N, device=self.device, dtype=torch.uint8)

    @classmethod
    def from_compiled(cls, num_envs: int, md: abi.ModelDesc, song: music.SongTables, tc: abi.TaskCfg, device=None,
                      seed: int = 0, env_offset: int = 0) -> "BatchedPianoEnv":
        """A handle on ``compile_task``'s outputs as given - e.g. with a field of ``tc`` edited
        (tests, studies). No augmentations: they need the song as notes."""
        # .task restates what tc carries (the model's options are not recoverable from md)
        task = TaskConfig(n_steps_lookahead=tc.n_steps_lookahead, wrong_press_termination=bool(tc.wrong_press_termination),
                          disable_forearm_reward=not tc.forearm_reward, energy_penalty_coef=tc.energy_penalty_coef,
                          randomize_hand_positions=bool(tc.randomize_hand_positions), solver_refine=tc.solver_refine,
                          solver_iterations=tc.solver_iterations or None, max_contacts=tc.max_contacts,
                          physics_timestep=md.timestep, control_timestep=md.timestep * md.n_substeps,
                          hand_side={abi.HAND_BOTH: None, abi.HAND_RIGHT: "right", abi.HAND_LEFT: "left"}[tc.hand_side],
                          observables=[n for i, n in enumerate(abi.OBSERVABLES) if tc.observables >> i & 1] or None)
        return cls(num_envs, song, task, device=device, seed=seed, env_offset=env_offset, _compiled=(md, song, tc))

    def _set_augmentations(self, midi) -> None:
        """TaskConfig.augmentations -> ps_set_augmentations: the bank (the initial song, then
        MidiSelect's), the variation list and T_cap, the rows the longest song takes at the largest
        stretch factor."""
        augs = variations.check(self.task.augmentations)
        if isinstance(midi, music.SongTables):
            raise TypeError("augmentations need the song as a NoteSequence or MIDI path, not as SongTables")
        songs = variations.bank(initial_sequence(midi, self.task), augs)
        for s in songs[1:]:
            # fingering_reward and obs_dim are fixed from the constructor's song
            # (piano_with_shadow_hands.py:110-112)
            if s.has_fingering() != songs[0].has_fingering():
                raise ValueError("MidiSelect: every song must agree with the task's song on has_fingering() "
                                 f"({songs[0].has_fingering()}); {s.title!r} does not")
        flats = [music.FlatSong.of(s) for s in songs]
        dt, buf = self.task.control_timestep, self.task.initial_buffer_time
        fmax = variations.max_stretch(augs)
        self.T_cap = max(int(f.total_time * fmax * (1.0 / dt) + 1) for f in flats) + int(round(buf / dt))
        bank = (abi.AugSong * len(flats))()
        for i, f in enumerate(flats):
            C.memmove(C.addressof(bank[i]), C.addressof(f), C.sizeof(abi.AugSong))
        var = (abi.Variation * max(1, len(augs)))(*[abi.Variation(v.kind, v.prob, v.range) for v in augs])
        desc = abi.AugmentDesc(n_songs=len(flats), songs=bank, n_variations=len(augs), variations=var, dt=dt,
                               initial_buffer_time=buf, T_cap=self.T_cap,
                               max_bytes=int(self.task.augmentation_max_bytes))
        _lib.check(_lib.load().ps_set_augmentations(self._h, C.addressof(desc)))
        self.augmentations, self.songs = augs, songs

    # -- lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.load().ps_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    # -- core API (device tensors, asynchronous on the current stream)
    def reset(self, mask=None):
        torch = self._torch
        mptr = None
        if mask is not None:
            self._mask = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            mptr = self._mask.data_ptr()
        _lib.check(_lib.load().ps_reset(self._h, mptr, self.obs.data_ptr(), self.stream))
        if mask is None:
            self.step_type.fill_(abi.FIRST)
        return self.obs

    def step(self, action):
        torch = self._torch
        a = torch.as_tensor(action, device=self.device, dtype=torch.float32)
        if a.shape != (self.num_envs, self.action_dim):
            raise ValueError(f"action must be [{self.num_envs}, {self.action_dim}], got {tuple(a.shape)}")
        a = a.contiguous()
        self._action = a  # keep alive until the kernel ran
        _lib.check(_lib.load().ps_step(self._h, a.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(),
                                       self.discount.data_ptr(), self.step_type.data_ptr(), self.stream))
        return self.obs, self.reward, self.discount, self.step_type

    def get_state(self) -> Dict[str, Any]:
        torch = self._torch
        N = self.num_envs
        out = dict(qpos=torch.empty(N, abi.NV, device=self.device), qvel=torch.empty(N, abi.NV, device=self.device),
                   qacc_ws=torch.empty(N, abi.NV, device=self.device), ctrl=torch.empty(N, abi.NU, device=self.device),
                   sustain=torch.empty(N, device=self.device),
                   t_idx=torch.empty(N, device=self.device, dtype=torch.int32),
                   last=torch.empty(N, device=self.device, dtype=torch.uint8))
        _lib.check(_lib.load().ps_get_state(self._h, *(out[k].data_ptr() for k in
                                                      ("qpos", "qvel", "qacc_ws", "ctrl", "sustain", "t_idx", "last")),
                                            self.stream))
        return out

    def set_state(self, state: Dict[str, Any]):
        torch = self._torch
        kinds = dict(qpos=torch.float32, qvel=torch.float32, qacc_ws=torch.float32, ctrl=torch.float32,
                     sustain=torch.float32, t_idx=torch.int32, last=torch.uint8)
        keep = {}
        for k, dt in kinds.items():
            if k in state and state[k] is not None:
                keep[k] = torch.as_tensor(state[k], device=self.device).to(dt).contiguous()
        ptr = lambda k: keep[k].data_ptr() if k in keep else None
        _lib.check(_lib.load().ps_set_state(self._h, *(ptr(k) for k in kinds), self.stream))
        self._keep = keep

    def set_applied(self, qfrc):
        torch = self._torch
        if qfrc is None:
            _lib.check(_lib.load().ps_set_applied(self._h, None, self.stream))
            return
        t = torch.as_tensor(qfrc, device=self.device, dtype=torch.float32).contiguous()
        _lib.check(_lib.load().ps_set_applied(self._h, t.data_ptr(), self.stream))
        self._applied = t

    def reward_terms(self):
        t = self._torch.empty(self.num_envs, abi.NTERMS, device=self.device)
        _lib.check(_lib.load().ps_reward_terms(self._h, t.data_ptr(), self.stream))
        return t

    def fingertips(self):
        t = self._torch.empty(self.num_envs, 2, 5, 3, device=self.device)
        _lib.check(_lib.load().ps_fingertips(self._h, t.data_ptr(), self.stream))
        return t

    def contact_count(self):
        t = self._torch.empty(self.num_envs, device=self.device, dtype=self._torch.int32)
        _lib.check(_lib.load().ps_contact_count(self._h, t.data_ptr(), self.stream))
        return t

    def record_contacts(self, on: bool = True) -> None:
        """Keep each step's contact list for contacts() (ps_record_contacts; off by default)."""
        _lib.check(_lib.load().ps_record_contacts(self._h, 1 if on else 0))

    def contacts(self):
        """-> list per env of (kind, key, g1, g2, dist, pos[3], normal[3]) of the last step's
        task-layer collision pass (physics.data.contact); needs record_contacts()."""
        raw = self._torch.empty(self.num_envs, abi.MAX_CONTACTS_LIMIT, 17, device=self.device, dtype=self._torch.float32)
        _lib.check(_lib.load().ps_contacts(self._h, raw.data_ptr(), self.stream))
        self._torch.cuda.synchronize(self.device)
        f = raw.cpu().numpy()
        ints = f.view(np.int32)
        n = self.contact_count().cpu().numpy()
        out = []
        for e in range(self.num_envs):
            out.append([(int(ints[e, c, 13]), int(ints[e, c, 14]), int(ints[e, c, 15]), int(ints[e, c, 16]),
                         float(f[e, c, 12]), f[e, c, 0:3].copy(), f[e, c, 3:6].copy()) for c in range(n[e])])
        return out

    def musical_metrics(self):
        """-> (episode [N, 6] f32, episodes [N] i32): each env's last finished episode's mean
        precision / recall / F1 / sustain_precision / sustain_recall / sustain_f1
        (MidiEvaluationWrapper, wrappers/evaluation.py:114-177) and its finished-episode count."""
        torch = self._torch
        ep = torch.empty(self.num_envs, abi.NMUSIC, device=self.device)
        cnt = torch.empty(self.num_envs, device=self.device, dtype=torch.int32)
        _lib.check(_lib.load().ps_musical_metrics(self._h, ep.data_ptr(), cnt.data_ptr(), self.stream))
        return ep, cnt

    def warnings(self):
        """[N, 3] int32: each env's mj_checkPos / mj_checkVel / mj_checkAcc resets since create
        (ps_warnings). MuJoCo resets the data of a diverged env and raises the warning that
        dm_control turns into ``PhysicsError``; the kernel does the reset per env and counts."""
        t = self._torch.empty(self.num_envs, abi.NWARN, device=self.device, dtype=self._torch.int32)
        _lib.check(_lib.load().ps_warnings(self._h, t.data_ptr(), self.stream))
        return t

    def solver_stats(self):
        """[N, 7] int32 counters of each env's last step (PS_STAT_*): Newton iterations, substeps
        at the contact cap, substeps at the Newton iteration cap, most contact rows, substeps with
        the hands coupled, substeps with a non-positive Hessian pivot, most coupled dofs of both
        hands in a substep."""
        t = self._torch.empty(self.num_envs, abi.NSTATS, device=self.device, dtype=self._torch.int32)
        _lib.check(_lib.load().ps_solver_stats(self._h, t.data_ptr(), self.stream))
        return t

    def hand_offset(self):
        """-> (dy [N] f32, episodes [N] i32): randomize_hand_positions' y shift of both hands this
        episode (piano_with_shadow_hands.py:491-499) and each env's resets so far."""
        torch = self._torch
        dy = torch.empty(self.num_envs, device=self.device)
        ep = torch.empty(self.num_envs, device=self.device, dtype=torch.int32)
        _lib.check(_lib.load().ps_get_hand_offset(self._h, dy.data_ptr(), ep.data_ptr(), self.stream))
        return dy, ep

    def set_hand_offset(self, dy):
        t = self._torch.as_tensor(dy, device=self.device, dtype=self._torch.float32).contiguous()
        _lib.check(_lib.load().ps_set_hand_offset(self._h, t.data_ptr(), self.stream))
        self._dy = t

    def _augmented(self) -> None:
        if self.augmentations is None:
            raise _lib.PianosimError("the env has no augmentations (TaskConfig(augmentations=[...]))")

    def augmentation(self) -> Dict[str, Any]:
        """This episode's draw of each env (ps_get_augmentation): ``song`` [N] i32 (index into
        ``self.songs``), ``factor`` [N] f64, ``shift`` [N] i32, the episode's length ``T`` [N] i32
        and ``fallbacks`` [N] i32 (draws that did not fit and played the selected song as given)."""
        self._augmented()
        torch = self._torch
        i = dict(device=self.device, dtype=torch.int32)
        out = dict(song=torch.empty(self.num_envs, **i), factor=torch.empty(self.num_envs, device=self.device,
                                                                            dtype=torch.float64),
                   shift=torch.empty(self.num_envs, **i), T=torch.empty(self.num_envs, **i),
                   fallbacks=torch.empty(self.num_envs, **i))
        _lib.check(_lib.load().ps_get_augmentation(self._h, *(out[k].data_ptr() for k in
                                                             ("song", "factor", "shift", "T", "fallbacks")),
                                                   self.stream))
        return out

    def set_augmentation(self, song, factor, shift) -> None:
        """Forces every env's draw ([N] each) and rebuilds its tables now; it holds until the
        env's next reset (ps_set_augmentation)."""
        self._augmented()
        torch = self._torch
        keep = (torch.as_tensor(song, device=self.device).to(torch.int32).contiguous(),
                torch.as_tensor(factor, device=self.device).to(torch.float64).contiguous(),
                torch.as_tensor(shift, device=self.device).to(torch.int32).contiguous())
        for t in keep:
            if t.shape != (self.num_envs,):
                raise ValueError(f"set_augmentation takes [{self.num_envs}] arrays, got {tuple(t.shape)}")
        _lib.check(_lib.load().ps_set_augmentation(self._h, *(t.data_ptr() for t in keep), self.stream))
        self._forced = keep

    def song_tables(self) -> Dict[str, Any]:
        """Each env's own tables (ps_get_song_tables): ``goal`` [N, T_cap, 89] f32, ``count``
        [N, T_cap], ``keys`` / ``fingers`` [N, T_cap, 16] i32; rows >= T of an env are stale."""
        self._augmented()
        torch = self._torch
        N, Tc = self.num_envs, self.T_cap
        i = dict(device=self.device, dtype=torch.int32)
        out = dict(goal=torch.empty(N, Tc, abi.NKEY + 1, device=self.device), count=torch.empty(N, Tc, **i),
                   keys=torch.empty(N, Tc, abi.MAX_NOTES, **i), fingers=torch.empty(N, Tc, abi.MAX_NOTES, **i))
        _lib.check(_lib.load().ps_get_song_tables(self._h, *(out[k].data_ptr() for k in
                                                            ("goal", "count", "keys", "fingers")), self.stream))
        return out

    # -- the piano's sound module (models/piano/midi_module.py): what each env played
    def record_midi(self, max_events: int = 2048, max_bytes: int = 0) -> None:
        """Records every env's NoteOn / NoteOff / SustainOn / SustainOff messages on the device,
        stamped with the physics substep they happened in (ps_record_midi). Two banks of
        ``max_events`` per env, the running episode and the last finished one: 16 KB per env at
        2048, 64 MB at 4096 envs. 0 turns recording off and frees them. Init-time: it
        synchronises; not under graph capture."""
        _lib.check(_lib.load().ps_record_midi(self._h, int(max_events), int(max_bytes)))
        self.midi_max_events = int(max_events)

    def _midi_which(self, which) -> int:
        if which not in ("current", "previous"):
            raise ValueError(f"which is 'current' or 'previous', not {which!r}")
        return 1 if which == "previous" else 0

    def midi_events(self, which: str = "current") -> Dict[str, Any]:
        """The running (``"current"``) or last finished (``"previous"``) episode of every env
        (ps_midi_events): ``events`` [N, max_events] int32 event words (music.decode_events; the
        first ``count`` of an env are valid, the others 0), ``count``, ``dropped`` (events that did
        not fit) and ``substeps`` (the episode's physics substeps so far) [N] int32."""
        w = self._midi_which(which)
        torch = self._torch
        i = dict(device=self.device, dtype=torch.int32)
        N = self.num_envs
        out = dict(events=torch.empty(N, getattr(self, "midi_max_events", 0), **i), count=torch.empty(N, **i),
                   dropped=torch.empty(N, **i), substeps=torch.empty(N, **i))
        _lib.check(_lib.load().ps_midi_events(self._h, w, *(out[k].data_ptr() for k in
                                                           ("events", "count", "dropped", "substeps")), self.stream))
        return out

    def midi_push(self, bits) -> None:
        """``MidiModule.after_substep`` on caller-supplied activations (ps_midi_push): ``bits``
        [N, rows, 3] event rows as music.pack_activations makes them, rows <= substeps per step."""
        torch = self._torch
        t = torch.as_tensor(bits, device=self.device).to(torch.int32).contiguous()
        if t.dim() != 3 or t.shape[0] != self.num_envs or t.shape[2] != 3:
            raise ValueError(f"bits must be [{self.num_envs}, rows, 3], got {tuple(t.shape)}")
        _lib.check(_lib.load().ps_midi_push(self._h, t.data_ptr(), int(t.shape[1]), self.stream))
        self._midi_bits = t  # keep alive until the kernel ran

    def _midi_env(self, i: int, which: str):
        # (an inspection call: it gathers every env's bank - [N, max_events] words, 32 MB at 4096
        # envs and 2048 events - and synchronises the device to read one env's)
        ev = self.midi_events(which)
        self._torch.cuda.synchronize(self.device)
        return (ev["events"][i].cpu().numpy(), int(ev["count"][i]), int(ev["dropped"][i]), int(ev["substeps"][i]))

    def midi_messages(self, i: int, which: str = "current") -> list:
        """Env ``i``'s messages (music.NoteOn / NoteOff / SustainOn / SustainOff) in the order the
        reference's ``MidiModule.get_all_midi_messages`` has them; time in seconds of physics.
        Not for the training loop: it copies all envs' banks and synchronises (``midi_events``
        stays on the device)."""
        words, count, _, _ = self._midi_env(i, which)
        return music.decode_events(words, count, self.model_desc.timestep)

    def performance(self, i: int, which: str = "current") -> music.NoteSequence:
        """Env ``i``'s episode as a NoteSequence (music.sequence_from_messages): a note still on
        at the episode's end (so far) is closed there; CC64 changes included; ``total_time`` the
        episode's. ``music.write_midi`` makes a ``.mid`` file of it."""
        words, count, _, substeps = self._midi_env(i, which)
        dt = self.model_desc.timestep
        return music.sequence_from_messages(music.decode_events(words, count, dt), substeps * dt,
                                            title=f"env {i} ({which})")

    # -- snapshots: save, restore and fork whole envs on the device (ps_snapshot_*)
    def snapshot(self, max_bytes: int = 0) -> "Snapshot":
        """A snapshot of every env as it is now: all the handle keeps per env (include/pianosim.h
        lists it) and the obs / reward / discount / step_type tensors. It belongs to this env and
        to its configuration now: ``record_midi`` / ``record_contacts`` afterwards invalidate it.
        ``max_bytes`` (0: no limit) bounds its device memory; more is an error."""
        return Snapshot(self, max_bytes)

    def restore(self, snap: "Snapshot", src=None) -> None:
        """Puts the envs back where ``snap`` has them. ``src`` None: every env takes its own row
        (a replay from here repeats bit for bit). ``src`` [N] int32: env i takes env ``src[i]``'s row
        - the fork; -1 leaves env i as it is, and so does any other index outside [0, N), which
        ``snap.n_bad`` (a device int32) counts. Forked envs keep their own ids, so with
        ``randomize_hand_positions`` or augmentations they draw differently at their next reset.
        Asynchronous on the current stream."""
        if not isinstance(snap, Snapshot) or snap._s is None:
            raise _lib.PianosimError("restore needs an open Snapshot")
        torch = self._torch
        sptr = nptr = None
        if src is not None:
            s = torch.as_tensor(src, device=self.device).to(torch.int32).contiguous()
            if s.shape != (self.num_envs,):
                raise ValueError(f"src must be [{self.num_envs}], got {tuple(s.shape)}")
            snap._src = s  # keep alive until the kernel ran
            snap.n_bad.zero_()
            sptr, nptr = s.data_ptr(), snap.n_bad.data_ptr()
        _lib.check(_lib.load().ps_snapshot_restore(self._h, snap._s, sptr, nptr, self.stream))
        # the caller-owned tensors, gathered the same way
        if src is None:
            for name, t in snap._outs.items():
                getattr(self, name).copy_(t)
            return
        ok = (s >= 0) & (s < self.num_envs)
        idx = torch.where(ok, s, torch.zeros_like(s)).long()
        for name, t in snap._outs.items():
            cur = getattr(self, name)
            cur.copy_(torch.where(ok.view(-1, *([1] * (cur.dim() - 1))), t.index_select(0, idx), cur))

    # -- rendering (ps_render; rendering.py)
    def render(self, camera="closeup", height: int = 240, width: int = 320, envs=None, depth: bool = False,
               segmentation: bool = False, change_color_on_activation: bool = False, colorize: Optional[bool] = None):
        """The envs ``envs`` (None: all N) ray-cast through ``camera`` (a name or index of
        ``rendering.CAMERAS``, or a ``rendering.Camera``) on the current stream: one tensor, uint8
        ``[n, H, W, 3]``, or float32 depth / int32 segmentation ``[n, H, W]`` (``rendering.render``)."""
        from . import rendering
        return rendering.render(self, camera, height, width, envs, depth, segmentation, change_color_on_activation,
                                colorize)

    def obs_dict(self, obs=None) -> Dict[str, Any]:
        obs = self.obs if obs is None else obs
        return {k: obs[:, s] for k, s in self.obs_slices.items()}

    # -- specs (dm_env)
    def observation_spec(self) -> Dict[str, Array]:
        return {k: Array((s.stop - s.start,), np.float64, k) for k, s in self.obs_slices.items()}

    def action_spec(self) -> BoundedArray:
        n = self.action_dim
        if self.canonical_actions:
            return BoundedArray((n,), np.float32, -np.ones(n, np.float32), np.ones(n, np.float32), "action")
        return BoundedArray((n,), np.float32, self.action_lo.astype(np.float32),
                            self.action_hi.astype(np.float32), "action")


class Snapshot:
    """One saved copy of every env of a :class:`BatchedPianoEnv` (``env.snapshot()``): the
    library's rows (ps_snapshot_*) and clones of the env's obs / reward / discount / step_type
    tensors. ``save()`` overwrites it with the envs as they are now; ``env.restore(snap, src)``
    reads it; ``close()`` frees it (before the env is closed)."""

    def __init__(self, env: BatchedPianoEnv, max_bytes: int = 0):
        self._env, self._s, self._src = env, None, None
        s = C.c_void_p()
        _lib.check(_lib.load().ps_snapshot_create(env._h, int(max_bytes), C.byref(s)))
        self._s = s
        self.bytes = int(_lib.load().ps_snapshot_bytes(s))
        self.n_bad = env._torch.zeros(1, device=env.device, dtype=env._torch.int32)
        self._outs = {k: env._torch.empty_like(getattr(env, k)) for k in ("obs", "reward", "discount", "step_type")}
        try:
            self.save()
        except Exception:
            self.close()
            raise

    def save(self) -> "Snapshot":
        if self._s is None:
            raise _lib.PianosimError("the snapshot is closed")
        env = self._env
        _lib.check(_lib.load().ps_snapshot_save(env._h, self._s, env.stream))
        for k, t in self._outs.items():
            t.copy_(getattr(env, k))
        return self

    def close(self) -> None:
        if self._s is not None:
            _lib.load().ps_snapshot_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- reference surfaces
class _EnvView:
    """``vec_env.envs[i]``: per-env dm_env views (specs; reset/step of that slot)."""

    def __init__(self, parent: "VectorizedPianoEnv", i: int):
        self._p, self._i = parent, i

    def observation_spec(self):
        return self._p._core.observation_spec()

    def action_spec(self):
        return self._p._core.action_spec()


class VectorizedPianoEnv:
    """Drop-in for ``parallelized_base_v2.VectorizedPianoEnv`` (parallelized_base_v2.py:21-67).

    ``reset()`` returns ``{key: [N, d]}``; ``step(actions[N, 45])`` ([N, 23] with ``hand_side``) (canonical [-1, 1], as
    after the reference's per-env ``CanonicalSpecWrapper``) returns ``(obs, rewards, dones)``.
    With ``return_numpy=True`` the outputs are numpy arrays like the reference's; otherwise
    they are torch-ROCm tensors that never leave HBM. The task kwargs default to the ones
    the reference hard-codes (parallelized_base_v2.py:28-39).
    """

    def __init__(self, num_envs: int, midi_sequence, return_numpy: bool = False, device=None, seed: int = 0,
                 **task_kwargs):
        kw = dict(n_steps_lookahead=1, trim_silence=True, wrong_press_termination=False,
                  initial_buffer_time=0.0, disable_fingering_reward=False, disable_forearm_reward=False,
                  disable_colorization=False, disable_hand_collisions=False)
        kw.update(task_kwargs)
        self.num_envs = num_envs
        self._core = BatchedPianoEnv(num_envs, midi_sequence, TaskConfig(**kw), device=device, seed=seed)
        self.return_numpy = return_numpy
        self.envs = [_EnvView(self, i) for i in range(num_envs)]
        self.observation_spec = self._core.observation_spec()
        self.action_spec = self._core.action_spec()

    @property
    def core(self) -> BatchedPianoEnv:
        return self._core

    def _obs(self, obs):
        # The reference returns fresh arrays each call (parallelized_base_v2.py:60-67); the
        # core's obs / reward buffers are reused by the next step, so the torch mode returns a
        # copy (one [N, obs_dim] device copy per step) that a driver may keep across steps.
        if self.return_numpy:
            flat = obs.detach().cpu().numpy().astype(np.float64)
        else:
            flat = obs.clone()
        return {k: flat[:, s] for k, s in self._core.obs_slices.items()}

    def reset(self):
        return self._obs(self._core.reset())

    def step(self, actions):
        obs, rew, disc, st = self._core.step(actions)
        obs_d = self._obs(obs)
        dones = st == abi.LAST
        if self.return_numpy:
            return obs_d, rew.detach().cpu().numpy().astype(np.float64), dones.cpu().numpy()
        return obs_d, rew.clone(), dones


class PhysicsError(RuntimeError):
    """dm_control's ``control.PhysicsError``: the simulation diverged (MuJoCo's mj_checkPos /
    mj_checkVel / mj_checkAcc warning: a NaN or |x| > 1e10 qpos, qvel or qacc)."""


_WARN_NAMES = ("mjWARN_BADQPOS", "mjWARN_BADQVEL", "mjWARN_BADQACC")


class Environment:
    """Single-env dm_env facade (``composer_utils.Environment`` + ``CanonicalSpecWrapper``).

    Physics errors follow ``composer.Environment.step``: the kernel resets a diverged env's
    physics and counts the warning (ps_warnings); with ``raise_exception_on_physics_error``
    (composer's default, True) the step raises ``PhysicsError``, otherwise it logs the warning
    and ends the episode with reward 0 and discount 0, and the next step resets."""

    def __init__(self, midi, task: Optional[TaskConfig] = None, device=None, seed: int = 0,
                 raise_exception_on_physics_error: bool = True):
        self._core = BatchedPianoEnv(1, midi, task, device=device, seed=seed)
        self._raise = raise_exception_on_physics_error
        self._warn = np.zeros(abi.NWARN, np.int64)
        self._reset_next = False

    def _obs(self, obs):
        return {k: v[0].detach().cpu().numpy() for k, v in self._core.obs_dict(obs).items()}

    def reset(self) -> TimeStep:
        self._reset_next = False
        obs = self._core.reset()
        self._warn = self._core.warnings()[0].cpu().numpy().astype(np.int64)
        return TimeStep(StepType.FIRST, None, None, self._obs(obs))

    def step(self, action) -> TimeStep:
        if self._reset_next:
            return self.reset()
        a = self._core._torch.as_tensor(np.asarray(action, np.float32).reshape(1, -1), device=self._core.device)
        obs, rew, disc, st = self._core.step(a)
        o = self._obs(obs)
        w = self._core.warnings()[0].cpu().numpy().astype(np.int64)
        new = w - self._warn
        self._warn = w
        if new.any():
            msg = "Physics state is invalid. Warning(s) raised: " + ", ".join(
                n for n, c in zip(_WARN_NAMES, new) if c > 0)
            if self._raise:
                raise PhysicsError(msg)
            import logging
            logging.warning(msg)
            self._reset_next = True
            return TimeStep(StepType.LAST, 0.0, 0.0, o)
        t = StepType(int(st[0]))
        if t == StepType.FIRST:
            return TimeStep(t, None, None, o)
        return TimeStep(t, float(rew[0]), float(disc[0]), o)

    def observation_spec(self):
        return self._core.observation_spec()

    def action_spec(self):
        return self._core.action_spec()

    @property
    def core(self):
        return self._core

    @property
    def physics(self):
        """``environment.physics``: ``physics.render(height, width, camera_id, depth, segmentation)``."""
        from . import rendering
        return rendering.Physics(self._core)


DEBUG = ["RoboPianist-debug-TwinkleTwinkleLittleStar-v0"]
_DEBUG_SONGS = {"RoboPianist-debug-TwinkleTwinkleLittleStar-v0": music.twinkle_twinkle_little_star_one_hand}


def song_for(environment_name: str, midi_file=None) -> music.NoteSequence:
    if midi_file is not None:
        return music.parse_midi(midi_file)
    if environment_name not in _DEBUG_SONGS:
        raise ValueError(f"Unknown environment {environment_name}. Available environments: {DEBUG}")
    return _DEBUG_SONGS[environment_name]()


def load(environment_name: str, midi_file=None, seed=None, stretch: float = 1.0, shift: int = 0, task_kwargs=None,
         device=None) -> Environment:
    """``robopianist.suite.load`` (suite/__init__.py:50-93) for the debug songs / MIDI files;
    ``stretch`` then ``shift`` are applied to the song as ``music.load`` does
    (music/__init__.py:92)."""
    song = music.transpose(music.stretch(song_for(environment_name, midi_file), stretch), shift)
    return Environment(song, TaskConfig(**(task_kwargs or {})), device=device, seed=0 if seed is None else int(seed))
