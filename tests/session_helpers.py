"""The session tests' model, step vocabulary and expectation (tests/test_session_model.py on the CPU, tests/test_gpu_session.py on the GPU).

A frame depends on the context's CURRENT state alone, never on the calls that led there: that is what include/vr_hip.h promises, and what
the feature files — each of which loads a scene, sets one feature's state, renders and resets — do not check.  Here a small model of the
context's LOGICAL state (SessionModel: one value per component, and the value it had before) is driven in lockstep with a real context
through long seeded sequences of setters and frames (sequences()), and every frame, or documented refusal, is held against what the
existing restatements (the *Ref classes of tests/*_helpers.py) give for the model's current state and nothing else (expected()).

The model states the drop and survive rules as the header words them, not as vr_hip_api.cpp implements them; READS, the table of which
components a frame kind reads, is read off the header too.  A kind that ignores a component is checked for free: its restatement never
sees it.  A plain module: no fixtures; the volumes, functions and tables come from a World built on the `vr` and `oracle` fixtures."""
import copy
import os

import numpy as np

import feature_random as fr
from backdrop_helpers import BackdropRef, synthetic_layer
from clip_helpers import CLIPS, IDENTITY, ClipRef
from depth_helpers import DepthRef
from fused_helpers import HOT, HOT_OPEN, INSIDE, FusedRef, bits_of, fused_esl
from gpu_feature import MAPPINGS, PLANES, SCHEDULINGS, WIDES
from iso_helpers import depth_bits
from label_helpers import LabelRef, constant_table, random_labels
from label_helpers import table as kinds_table
from light_helpers import PHONG
from section_helpers import SectionRef, unit
from shadow_helpers import CUTOFF, LIGHTS, ShadowRef
from slab_helpers import POINT, SLAB
from tf2d_helpers import Tf2dRef, choose_g_scale, esl_of, structured_table

SESSION_STREAM = 12                                     # np.random.default_rng([fr.SEED, 12, k]): streams 0-11 are taken by the feature files
OK, INVALID, NOT_READY = 0, 1, 5                        # vr_status
SIZE = fr.EDGE_SIZE                                     # every frame is 48 x 40
WINDOWS = ((48, 40), (64, 56), (96, 80))                # the window buffer: never smaller than a frame
PICKS = tuple((x, y) for y in (3, 12, 20, 28, 36) for x in (4, 12, 20, 28, 36, 44))

# ---- the frame kinds and what they read (include/vr_hip.h) -----------------------------------------------------------------------------

KINDS = ("volume", "mip", "iso", "backdrop", "hybrid", "section", "section_in_volume", "depth", "pick", "labelled", "tf2d", "fused")
# the kinds that run a composite pass with the context's lighting and shadow: "composite as before with one addition / replacement"
# (vr_hip_set_shadow, vr_hip_set_lighting), the backdrop ("with the context's clip, shadow, lighting and pre-integration"), the two composed
# forms ("the composite pass sees all of them") and step 2 of the labelled, tf2d and fused contracts ("under the context's clip ...,
# gradient lighting and shadow")
SHADED = ("volume", "backdrop", "hybrid", "section_in_volume", "labelled", "tf2d", "fused")
# pre-integration: the composite and what runs a composite pass, and step 3 of the depth contract (a pick is a depth frame's pixel); the
# labelled, tf2d and fused frames are refused under it, MIP, isosurface and section "IGNORE the state"
SLABBED = ("volume", "backdrop", "hybrid", "section_in_volume", "depth", "pick")
READS = {
    "volume": KINDS,
    # "independent of the 1-D transfer function" (tf2d, step 1) — but for the light grid, which is "built from the 1-D transfer function" (step 9)
    "tf": tuple(k for k in KINDS if k != "tf2d"),
    "clip": KINDS,                                      # "applies to every later composite, MIP and isosurface frame"; sections, depth, labelled, tf2d, fused: step 1 / 2 of each
    "lighting": SHADED,
    "shadow": SHADED,
    "preint": SLABBED,
    "labels": ("labelled",),                            # "every other entry point ignores both"
    "label_table": ("labelled",),
    "tf2d": ("tf2d",),                                  # "every other entry point ignores it"
    "second": ("fused",),                               # "Every other entry point ignores all of this"
    "second_tf": ("fused",),
}
PAIRS = tuple((c, k) for c in READS for k in READS[c])
STATE = tuple(READS)                                    # the components a frame can see
KNOBS = ("layout", "wide", "plane", "column_copy", "run_flavour", "mapping", "scheduling")
KNOB_DEFAULTS = {"layout": 1, "wide": 0, "plane": -1, "column_copy": 0, "run_flavour": 0, "mapping": (-1, 0, 0), "scheduling": 1}
PER_SAMPLE = ("labelled", "tf2d", "fused")              # refused while pre-integration is on
REFUSALS = ("labelled without labels", "fused without B", "fused without B's function", "tf2d without a table", "labelled under pre-integration",
            "tf2d under pre-integration", "fused under pre-integration", "tf2d NEAREST", "fused NEAREST", "composite NEAREST under a state")

# ---- the pools ---------------------------------------------------------------------------------------------------------------------------

# name -> (shape x y z, dtype, mirrored): two of equal dims and type but different contents (the reused allocations of the labels and of B,
# the same-dims set_volume), other dims with ragged last bricks and the table pad, the other voxel size, an extent of 1
POOL = {"a": ((9, 9, 9), "uint8", False), "a2": ((9, 9, 9), "uint8", True), "ragged": ((33, 8, 16), "uint8", False),
        "u16": ((17, 31, 2), "uint16", False), "flat": ((7, 9, 1), "uint8", False)}
GENERATED = (("noise", 12, 3, 1), ("shell", 16, 1, 1), ("noise", 9, 5, 2))       # vr_hip_generate_volume: kind, n, seed, bytes per voxel
CLIP_POOL = ("both", "box", "plane")
LIGHTING_POOL = (PHONG, (0.0, 1.0, 0.0, 0), (0.1, 0.3, 1.0, 10))
# (light, S, step, strength, sampling): the second differs from the first in the strength alone — the grid stays
SHADOW_POOL = ((LIGHTS["inside"], 5, 0.125, 1.0, 1), (LIGHTS["inside"], 5, 0.125, 0.5, 1), (LIGHTS["top"], 9, 0.09375, 0.75, 2))
SECTIONS = ((unit((0.2, -0.1, 1.0)) + (0.0,), 0.0, "point", None), (unit((1.0, 1.0, 1.0)) + (0.1,), 0.25, "mean", None),
            (unit((1.0, -1.0, 0.5)) + (0.0,), 0.2, "max", None), (unit((0.2, -0.1, 1.0)) + (-0.2,), 0.0, "point", "grey"))
LABEL_TABLES = ("kinds", "faded")
SECOND_VARIANTS = ("mirror_xz", "mirror_y")
SECOND_TFS = ("hot", "open")


class Value:
    """one value of a component: a printable name and the data behind it"""

    def __init__(self, name, data):
        self.name, self.data = name, data

    def __repr__(self):
        return self.name


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


class World:
    """Everything a step names, built once per (vr, oracle) and kept: the restatements cache by the arrays' addresses."""
    _instances = {}

    @classmethod
    def instance(cls, vr, oracle):
        key = (id(vr), id(oracle))
        if key not in cls._instances:
            cls._instances[key] = cls(vr, oracle)
        return cls._instances[key]

    def __init__(self, vr, oracle):
        self.vr, self.oracle = vr, oracle
        self._volumes, self._geometry, self._tfs, self._params, self._seconds, self._tf2d, self._layers = {}, {}, {}, {}, {}, {}, {}
        i = np.arange(128, dtype=np.float32)
        alt = np.stack([i / 127.0, 1.0 - i / 127.0, np.full(128, 0.5, np.float32), np.clip((i - 20.0) / 107.0, 0.0, 1.0) * 0.6], axis=1).astype(np.float32)
        alt[60:70, 3] = 0.0                             # a hole: values the default function shows and this one does not
        self.bases = (oracle.default_base_tf(), alt)
        self.label_tables = {"kinds": _frozen(kinds_table()), "faded": _frozen(constant_table(0.5, 0.5, (1.0, 0.0, 0.25)))}

    # -- volumes
    def volume(self, key):
        """key: a name of POOL, or ("gen", kind, n, seed, bytes per voxel)"""
        if key not in self._volumes:
            if isinstance(key, str):
                shape, dtype, mirrored = POOL[key]
                vox = fr.edge_volume(shape, dtype)
                if mirrored:
                    vox = vox[::-1, :, ::-1]
                name = key
            else:
                _, kind, n, seed, bpv = key
                vox, name = self.oracle.generate_volume(kind, n, seed, bpv), f"{kind}{n}s{seed}b{bpv}"
            self._volumes[key] = Value(name, _frozen(vox))
        return self._volumes[key]

    def geometry(self, volume):
        """(minmax, block dims, block size, ray step) of a volume"""
        if volume.name not in self._geometry:
            vox = volume.data
            mm, bd, bs = self.oracle.volume_minmax(vox)
            z, y, x = vox.shape
            self._geometry[volume.name] = (mm, bd, bs, fr.clamp_step(self.oracle.default_ray_step((x, y, z))))
        return self._geometry[volume.name]

    def tf(self, volume, base):
        """the premultiplied function of base `base` and its leaping bits for `volume`: Value((tf, esl))"""
        key = (volume.name, base)
        if key not in self._tfs:
            tf, esl = self.oracle.update_transfer_fn(self.bases[base], self.geometry(volume)[0])
            self._tfs[key] = Value(f"tf{base}@{volume.name}", (_frozen(tf), _frozen(esl)))
        return self._tfs[key]

    def tf2d(self, volume, base, g):
        """Value((table, g_scale, bits)): the structured table over base `base`, g_scale the volume's own (g = 0) or a quarter of it"""
        key = (volume.name, base, g)
        if key not in self._tf2d:
            table = structured_table(self.tf(volume, base).data[0])
            scale = choose_g_scale("session " + volume.name, volume.data) * (1.0, 0.25)[g]
            self._tf2d[key] = Value(f"tf2d{base}g{g}@{volume.name}", (table, float(scale), _frozen(esl_of(self.oracle, volume.data, table))))
        return self._tf2d[key]

    def labels(self, volume, salt):
        return Value(f"labels{salt}@{volume.data.shape[::-1]}", random_labels(volume.data, salt))

    def second(self, volume, variant):
        key = (volume.name, variant)
        if key not in self._seconds:
            vox = volume.data
            self._seconds[key] = Value(f"{variant}({volume.name})", _frozen(vox[::-1, :, ::-1] if variant == "mirror_xz" else vox[:, ::-1, :]))
        return self._seconds[key]

    def second_tf(self, which, esl_a, second):
        tf_b = HOT if which == "hot" else HOT_OPEN
        return Value(f"{which}&{second.name}", (tf_b, _frozen(fused_esl(esl_a, bits_of(self.oracle, second.data, tf_b)))))

    # -- frames
    def params(self, volume, view, sampling, march):
        """whole-frame parameters at 48 x 40 as fr.edge_scene makes them: the default mode (leaping, threshold 0.95) or the full march"""
        key = (volume.name, view, sampling, march)
        if key not in self._params:
            vr = self.vr
            _, bd, bs, step = self.geometry(volume)
            p = vr.VrParams()
            p.view = vr.benchmark_view(*SIZE, view)
            p.ray_step, p.light_kd = step, 0.7
            p.ray_threshold, p.esl = (1.0, 0) if march == "full" else (0.95, 1)
            p.esl_block_dims = int(bd)
            for j in range(3):
                p.esl_block_size[j] = float(bs[j])
            p.sampling = sampling
            self._params[key] = vr.whole_frame(p)
        return self._params[key]

    def level(self, volume):
        return 128.0 * (257.0 if volume.data.dtype == np.uint16 else 1.0)

    def window_of(self, volume, which):
        if which is None:
            return None
        return (2570.0, 64250.0) if volume.data.dtype == np.uint16 else (10.0, 250.0)


# ---- steps ------------------------------------------------------------------------------------------------------------------------------

class Step:
    """One call of a session: a setter (op, args) or a frame (op "frame": kind, view, sampling, march, entry, args)."""

    def __init__(self, op, **args):
        self.op, self.args = op, args

    def __getattr__(self, name):
        try:
            return self.__dict__["args"][name]
        except KeyError:
            raise AttributeError(name)

    @property
    def is_frame(self):
        return self.op == "frame"

    def line(self):
        return self.op + " " + " ".join(f"{k}={v}" for k, v in self.args.items())

    __repr__ = line


def frame(kind, view=0, sampling=1, march="default", entry="host", **args):
    return Step("frame", kind=kind, view=view, sampling=sampling, march=march, entry=entry, **args)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------

class SessionModel:
    """The context's logical state: one Value (or None: not set / off) per component of STATE, the value each had before its last change,
    the knobs, and what the testing aids of the ABI count.  apply(step) returns the status include/vr_hip.h promises for the call and, where
    that is VR_OK, changes the state as the header says the call changes it.

    `wrong`: a drop rule stated wrongly on purpose (tests/test_session_model.py: the sequences must notice) — "labels survive a volume",
    "B survives a volume", "tf2d goes with the volume", "label table goes with the volume", "B's function goes with B"."""

    def __init__(self, world, wrong=None):
        self.world, self.wrong = world, wrong
        self.now = {c: None for c in STATE}
        self.before = {c: None for c in STATE}
        self.changed = {c: None for c in STATE}          # index of the step that last changed the component
        self.arrival = None                              # how the resident volume arrived: host, device, generated
        self.window = None
        self.knobs = dict(KNOB_DEFAULTS)
        self.prepared = self.released = False
        self.refuse_env = False                          # VR_SECOND_COPY_REFUSE=1 in the environment
        self.refused_views = set()                       # views whose fused frames found B's copy refused; holds until B is set again
        self.shadow_stale, self.shadow_builds = True, 0
        self.counts = {k: 0 for k in ("lighting", "preint", "backdrop", "section", "depth", "labelled", "tf2d", "fused")}
        self.index = 0

    def fork(self, component=None):
        """a copy; with a component: that one set back to the value it had before its last change"""
        m = copy.copy(self)
        m.now, m.before, m.changed, m.knobs, m.counts = dict(self.now), dict(self.before), dict(self.changed), dict(self.knobs), dict(self.counts)
        m.refused_views = set(self.refused_views)
        if component is not None:
            m.now[component] = self.before[component]
        return m

    def _set(self, component, value):
        self.before[component], self.now[component], self.changed[component] = self.now[component], value, self.index - 1

    def __getattr__(self, name):
        if name in STATE:
            return self.__dict__["now"][name]
        raise AttributeError(name)

    # -- what the header says a new volume does
    def _new_volume(self, value, arrival):
        # "vr_hip_set_volume*, vr_hip_generate_volume drop them too" (labels, step 1); "drop it too" (B, step 1)
        if self.wrong != "labels survive a volume" or self.labels is None or self.labels.data.shape != value.data.shape:
            if self.labels is not None:
                self._set("labels", None)
        same = self.second is not None and self.second.data.shape == value.data.shape and self.second.data.dtype == value.data.dtype
        if self.second is not None and not (self.wrong == "B survives a volume" and same):
            self._set("second", None)
            self.refused_views = set()
        # "The table survives until it is replaced"; the 2-D table "survives a volume change"; "B's function and the bits survive a volume change"
        if self.wrong == "tf2d goes with the volume" and self.tf2d is not None:
            self._set("tf2d", None)
        if self.wrong == "label table goes with the volume" and self.label_table is not None:
            self._set("label_table", None)
        self._set("volume", value)
        self.arrival = arrival
        self.shadow_stale = True                         # "It goes stale ... on vr_hip_set_volume* / vr_hip_generate_volume"
        self.prepared = self.released = False            # "until the next set_volume"

    def apply(self, step):
        """the promised status of a setter step; the state changes where it is VR_OK"""
        w, op, a = self.world, step.op, step.args
        self.index += 1
        if op == "set_window":
            self.window = (a["w"], a["h"])
        elif op in ("set_volume", "set_volume_device"):
            self._new_volume(w.volume(a["key"]), "host" if op == "set_volume" else "device")
        elif op == "generate_volume":
            self._new_volume(w.volume(("gen", a["kind"], a["n"], a["seed"], a["bpv"])), "generated")
        elif op == "set_transfer_fn":
            self._set("tf", w.tf(self.volume, a["base"]))
            self.shadow_stale = True                     # "... on vr_hip_set_transfer_fn"
        elif op == "set_clip":
            new = Value(a["name"], CLIPS[a["name"]]) if a["name"] else None
            if (new and new.name) != (self.clip and self.clip.name):
                self._set("clip", new)
                self.shadow_stale = True                 # "... and on a vr_hip_set_clip that differs from the current clip"
        elif op == "set_lighting":
            new = None if a["i"] is None else Value(f"lighting{a['i']}", LIGHTING_POOL[a["i"]])
            if (new and new.name) != (self.lighting and self.lighting.name):
                self._set("lighting", new)
        elif op == "set_shadow":
            new = None if a["i"] is None else Value(f"shadow{a['i']}", SHADOW_POOL[a["i"]])
            if (new and new.name) != (self.shadow and self.shadow.name):
                old = self.shadow
                self._set("shadow", new)
                # "a vr_hip_set_shadow whose struct differs from the current one in more than `strength`"
                if new is not None and not (old is not None and old.data[:3] == new.data[:3] and old.data[4] == new.data[4]):
                    self.shadow_stale = True
        elif op == "set_preintegration":
            if bool(a["on"]) != bool(self.preint):
                self._set("preint", Value("slab", True) if a["on"] else None)
        elif op in ("set_labels", "set_labels_device"):
            self._set("labels", None if a["salt"] is None else w.labels(self.volume, a["salt"]))
        elif op == "set_label_table":
            self._set("label_table", None if a["name"] is None else Value(a["name"], w.label_tables[a["name"]]))
        elif op == "set_tf2d":
            self._set("tf2d", None if a["base"] is None else w.tf2d(self.volume, a["base"], a["g"]))
        elif op in ("set_second_volume", "set_second_volume_device"):
            self._set("second", None if a["variant"] is None else w.second(self.volume, a["variant"]))
            self.refused_views = set()                   # "a refusal holds until B is set again"
            if a["variant"] is None and self.wrong == "B's function goes with B" and self.second_tf is not None:
                self._set("second_tf", None)
        elif op == "set_second_transfer_fn":
            second = self.second if self.second is not None else w.second(self.volume, SECOND_VARIANTS[0])
            self._set("second_tf", w.second_tf(a["which"], self.tf.data[1], second))
        elif op == "refuse_second_copy":
            self.refuse_env = bool(a["on"])
        elif op == "prepare":
            # after a release: nothing is left to build where everything the policy has is resident
            self.prepared = self.prepared or self.knobs["layout"] == 1
        elif op == "release_linear_copy":
            if self.released:
                return OK
            # "Refused (VR_ERR_INVALID) when no brick copy is resident yet ... and while the index-arithmetic path is forced"
            if self.knobs["layout"] == 0 or self.knobs["wide"] == 1:
                return INVALID
            assert self.prepared, "release_linear_copy is modelled behind vr_hip_prepare alone: which copies frames have built is no logical state"
            self.released = True
        elif op == "download_shadow":
            if self.shadow is None:
                return NOT_READY                         # "VR_ERR_NOT_READY without a shadow"
            self._grid_read()
        elif op == "set_layout":
            if self.released:
                return NOT_READY                         # "vr_hip_set_layout / vr_hip_prepare return VR_ERR_NOT_READY until the next set_volume"
            self.knobs["layout"], self.prepared = a["v"], False
        elif op == "set_wide_addressing":
            if self.released and (a["v"] & 3) == 1:
                return NOT_READY                         # the index-arithmetic path reads the linear array
            self.knobs["wide"] = a["v"]
        elif op in ("set_brick_plane", "set_column_copy", "set_run_flavour", "set_tile_scheduling"):
            self.knobs[{"set_brick_plane": "plane", "set_column_copy": "column_copy", "set_run_flavour": "run_flavour", "set_tile_scheduling": "scheduling"}[op]] = a["v"]
        elif op == "set_tile_mapping":
            self.knobs["mapping"] = (a["lane_map"], a["px"], a["py"])
        else:
            raise ValueError(op)
        return OK

    # -- frames
    def refusal(self, f):
        """(status, which of REFUSALS) of a frame the header refuses in this state, (0, None) otherwise.  Where two refusals meet,
        VR_ERR_INVALID — the call can never succeed in this state of the knobs — goes before VR_ERR_NOT_READY."""
        nearest, k = f.sampling == 0, f.kind
        if nearest and k in ("tf2d", "fused"):
            return INVALID, f"{k} NEAREST"
        if nearest and k not in ("volume", "mip"):
            return INVALID, "other NEAREST"
        if nearest and k == "volume" and (self.shadow or self.lighting or self.preint):
            return INVALID, "composite NEAREST under a state"
        if k in PER_SAMPLE and self.preint:
            return INVALID, f"{k} under pre-integration"
        if k == "labelled" and self.labels is None:
            return NOT_READY, "labelled without labels"
        if k == "tf2d" and self.tf2d is None:
            return NOT_READY, "tf2d without a table"
        if k == "fused" and self.second is None:
            return NOT_READY, "fused without B"
        if k == "fused" and self.second_tf is None:
            return NOT_READY, "fused without B's function"
        return OK, None

    def _grid_read(self):
        if self.shadow_stale:
            self.shadow_builds += 1
            self.shadow_stale = False

    def count(self, f):
        """a frame that was launched: the counters of the testing aids, the light grid built where it was stale, the refused copy of B"""
        self.index += 1
        k, c = f.kind, self.counts
        if k in ("volume", "backdrop", "hybrid", "section_in_volume"):
            c["lighting"] += self.lighting is not None
            c["preint"] += self.preint is not None
        c["backdrop"] += k in ("backdrop", "hybrid", "section_in_volume")
        c["section"] += k in ("section", "section_in_volume")
        c["depth"] += {"depth": 1, "pick": len(PICKS)}.get(k, 0)
        for own in PER_SAMPLE:
            c[own] += k == own
        if k in SHADED and self.shadow is not None:
            self._grid_read()
        if k == "fused" and self.refuse_env:
            self.refused_views.add(f.view)

    def fused_layout(self, f):
        """what vr_launch_info::layout of a fused frame must say: "linear" while B's copy is refused, "bricks" on the defaults, None: not held"""
        if self.refuse_env or f.view in self.refused_views:
            return "linear"
        if self.knobs == KNOB_DEFAULTS and not self.refused_views:
            return "bricks"
        return None


# ---- the expectation ----------------------------------------------------------------------------------------------------------------------

class Want:
    """what a frame step must give: a status, and for VR_OK the buffers — rgba, depth, value, alpha, picks ([n, 10] float32: hit, k, value,
    alpha, position, voxel) —, None where the kind has none"""

    def __init__(self, status=OK, refusal=None, **buffers):
        self.status, self.refusal, self.buffers = status, refusal, buffers

    def differs(self, other):
        """elements that differ — pixels of the RGBA frame, bit patterns of the floats — or -1 where the statuses or the buffers do"""
        if self.status != other.status or set(self.buffers) != set(other.buffers):
            return -1
        n = 0
        for name, a in self.buffers.items():
            b = other.buffers[name]
            if a.shape != b.shape:
                return -1
            if name == "rgba":
                n += int((a != b).any(axis=-1).sum())
            elif name == "picks":
                n += int((depth_bits(a) != depth_bits(b)).any(axis=-1).sum())
            else:
                n += int((depth_bits(a) != depth_bits(b)).sum())
        return n


def expected(model, f):
    """The status, or the restatement's answer for the model's current state and nothing else."""
    status, which = model.refusal(f)
    if status:
        return Want(status, which)
    w, m = model.world, model
    vol, vox = m.volume, m.volume.data
    tf, esl = m.tf.data
    p = w.params(vol, f.view, f.sampling, f.march)
    clip = m.clip.data if m.clip else IDENTITY
    lighting = m.lighting.data if m.lighting else None
    cmode = SLAB if m.preint else POINT
    q, strength = None, 1.0
    if m.shadow and f.kind in SHADED:
        light, S, step, strength, sampling = m.shadow.data
        q = ShadowRef.instance().build(light, S, step, vox, tf, CUTOFF, sampling, clip=m.clip.data if m.clip else None)
    shading = (cmode, clip, lighting, q, strength)
    unskipped = fr.with_sampling(p, f.sampling, 0)      # the restatements of MIP and isosurface do not look at esl: one cache entry for both
    k = f.kind
    if k == "volume":
        if f.sampling == 0:
            return Want(rgba=ClipRef.instance().composite(p, vox, tf, esl, clip))
        return Want(rgba=BackdropRef.instance().render(p, vox, tf, esl, None, None, *shading))
    if k == "mip":
        return Want(rgba=ClipRef.instance().mip(unskipped, vox, tf, clip))
    if k == "iso":
        rgba, depth, _ = ClipRef.instance().iso(unskipped, vox, tf, w.level(vol), f.refine, clip)
        return Want(rgba=rgba, depth=depth)
    if k == "backdrop":
        ref = BackdropRef.instance()
        rgba, depth = layer_of(model, f)
        return Want(rgba=ref.render(p, vox, tf, esl, rgba, depth, *shading))
    if k == "hybrid":
        rgba, depth, _ = BackdropRef.instance().hybrid(p, vox, tf, esl, w.level(vol), f.refine, *shading)
        return Want(rgba=rgba, depth=depth)
    if k in ("section", "section_in_volume"):
        plane, half_width, mode, window = SECTIONS[f.section]
        window = w.window_of(vol, window)
        if k == "section":
            rgba, depth = SectionRef.instance().render(p, vox, tf, plane, half_width, mode, window, clip)[:2]
        else:
            rgba, depth, _ = SectionRef.instance().in_volume(p, vox, tf, esl, plane, half_width, mode, window, *shading)
        return Want(rgba=rgba, depth=depth)
    if k in ("depth", "pick"):
        d = DepthRef.instance().render(p, vox, tf, esl, f.opacity, f.mode, cmode, clip)
        if k == "depth":
            return Want(depth=d.depth, value=d.value, alpha=d.alpha)
        picks = np.zeros((len(PICKS), 10), np.float32)
        for i, (x, y) in enumerate(PICKS):
            picks[i, :4] = (float(d.depth[y, x] >= 0.0), d.depth[y, x], d.value[y, x], d.alpha[y, x])
            picks[i, 4:] = d.pick[y, x]
        return Want(picks=picks)
    if k == "labelled":
        entries = m.label_table.data if m.label_table else np.zeros((0, 5), np.float32)
        return Want(rgba=LabelRef.instance().render(p, vox, tf, esl, m.labels.data, entries, lighting, q, strength, clip).frame)
    if k == "tf2d":
        table, g_scale, bits = m.tf2d.data
        return Want(rgba=Tf2dRef.instance().render(p, vox, table, g_scale, bits, lighting, q, strength, clip).frame)
    if k == "fused":
        tf_b, bits = m.second_tf.data
        return Want(rgba=FusedRef.instance().render(p, vox, tf, bits, m.second.data, tf_b, f.mode, f.wa, f.wb, lighting, q, strength, clip).frame)
    raise ValueError(k)


def layer_of(model, f):
    """the synthetic layer of a backdrop step: backdrop_helpers.synthetic_layer for the model's volume, function and clip under the step's salt"""
    w = model.world
    tf, esl = model.tf.data
    clip = model.clip.data if model.clip else IDENTITY
    key = (model.volume.name, model.tf.name, model.clip.name if model.clip else None, f.view, f.sampling, f.march, f.salt)
    if key not in w._layers:
        w._layers[key] = synthetic_layer(BackdropRef.instance(), w.params(model.volume, f.view, f.sampling, f.march), model.volume.data, tf, esl, clip, salt=4000 + f.salt)
    return w._layers[key]


# ---- the sequences --------------------------------------------------------------------------------------------------------------------------

READER_OF = {"labels": "labelled", "label_table": "labelled", "tf2d": "tf2d", "second": "fused", "second_tf": "fused"}


class _Writer:
    """Writes one sequence: keeps a model in lockstep so that every step it draws is one the context can be given."""

    def __init__(self, world, k):
        self.world, self.rng, self.steps = world, np.random.default_rng([fr.SEED, SESSION_STREAM, k]), []
        self.model = SessionModel(world)

    def emit(self, step):
        self.steps.append(step)
        if step.is_frame:
            if self.model.refusal(step)[0] == OK:
                self.model.count(step)
            else:
                self.model.index += 1
        else:
            self.model.apply(step)
        return step

    def pick(self, pool):
        return pool[int(self.rng.integers(0, len(pool)))]

    def other(self, pool, current):
        """a member of the pool that is not the current one"""
        rest = [v for v in pool if v != current]
        return rest[int(self.rng.integers(0, len(rest)))]

    # -- frames
    def frame(self, kind, **fixed):
        rng = self.rng
        args = dict(view=int(self.pick(fr.EDGE_VIEWS)), sampling=int(self.pick((1, 2))), march=self.pick(("default", "full")),
                    entry="host" if kind == "pick" else self.pick(("host", "device")))
        if kind in ("iso", "hybrid"):
            args["refine"] = int(self.pick((0, 4)))
        if kind in ("hybrid", "section_in_volume"):
            args["own_depth"] = bool(rng.integers(0, 2))  # the device entry point with dev_depth NULL: the context-owned buffer
        if kind in ("section", "section_in_volume"):
            args["section"] = int(rng.integers(0, len(SECTIONS)))
        if kind in ("depth", "pick"):
            args["opacity"], args["mode"] = float(self.pick((0.1, 0.5))), self.pick(("first", "peak", "mean"))
        if kind == "backdrop":
            args["salt"] = int(rng.integers(0, 2))
        if kind == "fused":
            args["mode"] = self.pick(("sum", "over"))
            args["wa"], args["wb"] = self.pick(((1.0, 1.0), INSIDE))
        args.update(fixed)
        return self.emit(frame(kind, **args))

    def renderable(self, kind):
        """the state a frame of this kind needs, set where it is missing"""
        m = self.model
        if kind in PER_SAMPLE and m.preint:
            self.emit(Step("set_preintegration", on=0))
        if kind == "labelled" and m.labels is None:
            self.set_labels()
        if kind == "tf2d" and m.tf2d is None:
            self.change("tf2d")
        if kind == "fused":
            if m.second is None:
                self.set_second()
            if m.second_tf is None:
                self.change("second_tf")

    def set_labels(self, clear=False):
        cur = None if self.model.labels is None else int(self.model.labels.name[6])
        self.emit(Step(self.pick(("set_labels", "set_labels_device")), salt=None if clear else self.other((0, 1), cur)))

    def set_second(self, clear=False):
        cur = None if self.model.second is None else self.model.second.name.split("(")[0]
        self.emit(Step(self.pick(("set_second_volume", "set_second_volume_device")), variant=None if clear else self.other(SECOND_VARIANTS, cur)))

    def set_volume(self, key=None):
        cur = self.model.volume
        if key is None:
            names = [n for n in POOL if cur is None or n != cur.name]
            if self.rng.random() < 0.2:
                kind, n, seed, bpv = self.pick(GENERATED)
                return self.emit(Step("generate_volume", kind=kind, n=n, seed=seed, bpv=bpv))
            key = self.pick(names)
        return self.emit(Step(self.pick(("set_volume", "set_volume_device")), key=key))

    def change(self, component, clear=None):
        """one setter that changes the component: a new value, or — clear, or one time in four where it is set — its clear / drop"""
        m, rng = self.model, self.rng
        cur = m.now[component]
        if clear is None:
            clear = cur is not None and component not in ("volume", "tf", "second_tf") and rng.random() < 0.25
        if component == "volume":
            self.set_volume()
            if rng.random() < 0.5:                       # (the bits of the function then belong to the volume before: leaping is defined by the bits it is given)
                self.emit(Step("set_transfer_fn", base=0 if m.tf is None else int(m.tf.name[2])))
        elif component == "tf":
            self.emit(Step("set_transfer_fn", base=1 - int(cur.name[2]) if cur is not None and cur.name.endswith("@" + m.volume.name) else int(rng.integers(0, 2))))
        elif component == "clip":
            self.emit(Step("set_clip", name=None if clear else self.other(CLIP_POOL, cur and cur.name)))
        elif component == "lighting":
            self.emit(Step("set_lighting", i=None if clear else self.other((0, 1, 2), cur and int(cur.name[-1]))))
        elif component == "shadow":
            self.emit(Step("set_shadow", i=None if clear else self.other((0, 1, 2), cur and int(cur.name[-1]))))
        elif component == "preint":
            self.emit(Step("set_preintegration", on=0 if cur is not None else 1))
        elif component == "labels":
            self.set_labels(clear)
        elif component == "label_table":
            self.emit(Step("set_label_table", name=None if clear else self.other(LABEL_TABLES, cur and cur.name)))
        elif component == "tf2d":
            if clear:
                self.emit(Step("set_tf2d", base=None, g=None))
            else:
                options = [(b, g) for b in (0, 1) for g in (0, 1) if cur is None or cur.name != f"tf2d{b}g{g}@{m.volume.name}"]
                b, g = self.pick(options)
                self.emit(Step("set_tf2d", base=b, g=g))
        elif component == "second":
            self.set_second(clear)
        elif component == "second_tf":
            which = self.other(SECOND_TFS, cur and cur.name.split("&")[0]) if cur is not None and m.second is not None and cur.name.endswith("&" + m.second.name) \
                else self.pick(SECOND_TFS)
            self.emit(Step("set_second_transfer_fn", which=which))

    def knob(self):
        rng, m = self.rng, self.model
        which = self.pick(KNOBS + ("window", "prepare") + (("download_shadow",) if m.shadow is not None else ()))
        if which == "layout":
            self.emit(Step("set_layout", v=1 - m.knobs["layout"]))
        elif which == "wide":
            self.emit(Step("set_wide_addressing", v=self.other(WIDES, m.knobs["wide"])))
        elif which == "plane":
            self.emit(Step("set_brick_plane", v=self.other(PLANES, m.knobs["plane"])))
        elif which == "column_copy":
            self.emit(Step("set_column_copy", v=self.other((0, 1, 2), m.knobs["column_copy"])))
        elif which == "run_flavour":
            self.emit(Step("set_run_flavour", v=self.other((0, 1, 2), m.knobs["run_flavour"])))
        elif which == "mapping":
            lane_map, phase = (-1, (0, 0)) if m.knobs["mapping"][0] >= 0 and rng.random() < 0.5 else self.pick(MAPPINGS)
            self.emit(Step("set_tile_mapping", lane_map=lane_map, px=phase[0], py=phase[1]))
        elif which == "scheduling":
            self.emit(Step("set_tile_scheduling", v=self.other(SCHEDULINGS, m.knobs["scheduling"])))
        elif which == "window":
            w, h = self.other(WINDOWS, m.window)
            self.emit(Step("set_window", w=w, h=h))
        else:
            self.emit(Step(which))

    # -- the parts of a sequence
    def prologue(self, key="a"):
        self.emit(Step("set_window", w=SIZE[0], h=SIZE[1]))
        self.emit(Step("set_volume", key=key))
        self.emit(Step("set_transfer_fn", base=0))

    def everything_set(self):
        """labels, a table, B with its function, a 2-D table and a shadow in place"""
        m = self.model
        for component in ("labels", "label_table", "tf2d", "second", "second_tf", "shadow"):
            if m.now[component] is None:
                self.change(component, clear=False)
        if m.preint:
            self.emit(Step("set_preintegration", on=0))

    def transitions(self):
        """set -> clear -> set of every state that can be cleared, each followed by a frame that reads it; the three kinds of volume change
        with labels, B, a 2-D table and a shadow in place; a window grow between two host frames with depth"""
        for component in ("clip", "lighting", "shadow", "preint", "labels", "tf2d", "second"):
            reader = READER_OF.get(component, "volume")
            for clear in (False, True, False):
                self.change(component, clear=clear if component != "preint" else None)
                if not clear:
                    self.renderable(reader)
                self.frame(reader, sampling=1)
        for key in ("a2", "ragged", "u16"):               # the same dims and type with other contents, other dims, the other voxel size
            self.everything_set()
            for kind in ("labelled", "fused", "tf2d", "volume"):
                self.frame(kind, sampling=1)
            self.emit(Step("set_volume", key=key))
            for kind in ("labelled", "fused", "tf2d", "volume"):
                self.frame(kind, sampling=1)
            self.frame("mip", march="default")
            self.emit(Step("set_transfer_fn", base=0))
        for kind in ("iso", "hybrid", "depth"):
            self.emit(Step("set_window", w=SIZE[0], h=SIZE[1]))
            self.frame(kind, entry="host", sampling=1)
            self.emit(Step("set_window", w=WINDOWS[2][0], h=WINDOWS[2][1]))
            self.frame(kind, entry="host", sampling=1)

    def knob_sweep(self):
        """every value of PLANES, WIDES and SCHEDULINGS, both layouts, the column copies, the run flavours and six mappings, a frame behind each"""
        kinds = [k for k in KINDS if k not in PER_SAMPLE]
        n = 0

        def one(op, back, **args):
            nonlocal n
            self.emit(Step(op, **args))
            self.frame(kinds[n % len(kinds)])
            n += 1
            if back is not None:
                self.emit(Step(op, **back))
        for v in (0, 1):
            one("set_layout", None, v=v)
        for v in PLANES:
            one("set_brick_plane", None, v=v)
        self.emit(Step("set_brick_plane", v=-1))
        for v in WIDES:
            one("set_wide_addressing", None, v=v)
        self.emit(Step("set_wide_addressing", v=0))
        for v in SCHEDULINGS:
            one("set_tile_scheduling", None, v=v)
        self.emit(Step("set_tile_scheduling", v=1))
        for v in (1, 2, 0):
            one("set_column_copy", None, v=v)
        for v in (1, 2, 0):
            one("set_run_flavour", None, v=v)
        for lane_map, phase in MAPPINGS[::3]:
            one("set_tile_mapping", None, lane_map=lane_map, px=phase[0], py=phase[1])
        self.emit(Step("set_tile_mapping", lane_map=-1, px=0, py=0))

    def refusals(self):
        """every refusal expected() predicts, between two successful frames of another kind that are the same step"""
        m = self.model

        def refused(step_of, which):
            before = self.frame("mip", sampling=1, entry="host", view=1, march="full")
            f = step_of()
            assert m.refusal(f)[1] == which, (which, m.refusal(f))
            self.emit(frame(**before.args))
        for component in ("labels", "tf2d", "second"):
            if m.now[component] is None:
                self.change(component, clear=False)
        self.change("second_tf")
        if m.preint:
            self.emit(Step("set_preintegration", on=0))
        refused(lambda: self.frame("tf2d", sampling=0), "tf2d NEAREST")
        refused(lambda: self.frame("fused", sampling=0), "fused NEAREST")
        self.emit(Step("set_preintegration", on=1))
        for kind in PER_SAMPLE:
            refused(lambda: self.frame(kind, sampling=1), f"{kind} under pre-integration")
        refused(lambda: self.frame("volume", sampling=0), "composite NEAREST under a state")
        self.emit(Step("set_preintegration", on=0))
        self.set_labels(clear=True)
        refused(lambda: self.frame("labelled", sampling=2), "labelled without labels")
        self.emit(Step("set_tf2d", base=None, g=None))
        refused(lambda: self.frame("tf2d", sampling=2), "tf2d without a table")
        self.set_second(clear=True)
        refused(lambda: self.frame("fused", sampling=2), "fused without B")

    def without_second_tf(self):
        """B without a function: only a context that was never given one can show it"""
        self.set_second()
        before = self.frame("mip", sampling=1, entry="host", view=1, march="full")
        f = self.frame("fused", sampling=1)
        assert self.model.refusal(f)[1] == "fused without B's function"
        self.emit(frame(**before.args))

    def random(self, length, knobs=0.3):
        """change one component, then render several kinds that read it, knob changes in between"""
        rng = self.rng
        weights = {"volume": 3, "tf": 2, "clip": 2, "lighting": 2, "shadow": 2, "preint": 2, "labels": 1, "label_table": 1, "tf2d": 1, "second": 1, "second_tf": 1}
        names = list(weights)
        prob = np.array([weights[n] for n in names], float)
        prob /= prob.sum()
        while len(self.steps) < length:
            component = names[int(rng.choice(len(names), p=prob))]
            self.change(component)
            readers = list(READS[component])
            for i in rng.permutation(len(readers))[: int(rng.integers(2, 5))]:
                kind = readers[int(i)]
                if rng.random() < knobs:
                    self.knob()
                nearest = kind in ("volume", "mip") and rng.random() < 0.15
                if not nearest and rng.random() < 0.85:
                    self.renderable(kind)
                self.frame(kind, **({"sampling": 0} if nearest else {}))


LENGTHS = {"general0": 170, "general1": 210, "general2": 210, "release": 160, "refuse": 130}
NAMES = tuple(LENGTHS)
_sequences = {}


def sequence(world, name):
    """the step list of one sequence: deterministic in fr.SEED and the name's number"""
    if name in _sequences:
        return _sequences[name]
    k = NAMES.index(name)
    w = _Writer(world, k)
    if name == "general0":
        w.prologue("a")
        w.without_second_tf()
        w.transitions()
    elif name == "general1":
        w.prologue("ragged")
        w.knob_sweep()
    elif name == "general2":
        w.prologue("a2")
        w.refusals()
    elif name == "release":
        # prepare, release, what the header refuses until the next set_volume, every kind from the copies alone, then a new volume
        w.prologue("a")
        w.everything_set()
        w.emit(Step("set_layout", v=0))
        w.emit(Step("release_linear_copy"))             # refused: no brick copy is resident
        w.emit(Step("set_layout", v=1))
        w.emit(Step("prepare"))
        w.emit(Step("set_wide_addressing", v=1))
        w.emit(Step("release_linear_copy"))             # refused: the index-arithmetic path is forced
        w.emit(Step("set_wide_addressing", v=0))
        w.frame("mip", march="default", sampling=1)     # (its block maxima exist before the release; the second release below derives them itself)
        w.emit(Step("release_linear_copy"))
        for step in (Step("set_layout", v=0), Step("set_wide_addressing", v=1), Step("prepare"), Step("release_linear_copy")):
            w.emit(step)
        for kind in KINDS:
            w.frame(kind, sampling=1 + KINDS.index(kind) % 2)
        w.frame("mip", sampling=0, march="default")
        w.frame("volume", sampling=1, march="full", view=0)
        w.emit(Step("set_clip", name="box"))
        w.emit(Step("download_shadow"))
        for kind in SHADED:
            w.frame(kind, sampling=1)
        w.emit(Step("set_volume", key="ragged"))
        w.emit(Step("set_transfer_fn", base=1))
        w.emit(Step("prepare"))
        w.emit(Step("release_linear_copy"))             # (no MIP frame with esl on came before: the release derives the maxima)
        w.frame("mip", march="default", sampling=2)
        w.frame("mip", march="default", sampling=0)
        w.emit(Step("set_layout", v=0))                 # refused again
        w.emit(Step("set_volume_device", key="a2"))
        w.emit(Step("set_layout", v=0))                 # ... and not after the next set_volume
        w.frame("volume", sampling=1)
        w.emit(Step("set_layout", v=1))
    elif name == "refuse":
        w.prologue("a")
        w.everything_set()
        for view in fr.EDGE_VIEWS:
            w.frame("fused", view=view, sampling=1)
        w.emit(Step("refuse_second_copy", on=1))
        w.set_second()
        for view in fr.EDGE_VIEWS:
            w.frame("fused", view=view, sampling=1 + view % 2)
        w.frame("volume", sampling=1)
        w.emit(Step("refuse_second_copy", on=0))
        for view in fr.EDGE_VIEWS:
            w.frame("fused", view=view, sampling=2 - view % 2)      # refused, not retried
        w.set_second()
        for view in fr.EDGE_VIEWS:
            w.frame("fused", view=view, sampling=1)
    w.random(LENGTHS[name], knobs=0.3)
    if w.model.refuse_env:
        w.emit(Step("refuse_second_copy", on=0))
    _sequences[name] = w.steps
    return w.steps


def sequences(world):
    return {name: sequence(world, name) for name in NAMES}


def trace(steps, upto):
    return "\n".join(f"{i:4d}  {s.line()}" for i, s in enumerate(steps[: upto + 1]))


def walk(world, steps, wrong=None):
    """(index, step, model BEFORE a frame step / AFTER a setter step, promised status) of every step, the model counting as it goes"""
    model = SessionModel(world, wrong)
    for i, step in enumerate(steps):
        if step.is_frame:
            status = model.refusal(step)[0]
            yield i, step, model, status
            if status == OK:
                model.count(step)
            else:
                model.index += 1
        else:
            status = model.apply(step)
            yield i, step, model, status


# ---- a real context in lockstep (tests/test_gpu_session.py) ----------------------------------------------------------------------------

def session_renderer(device=0):
    """One renderer with every frame kind: the package keeps FusedRenderer and Tf2dRenderer in modules of their own, both plain extensions
    of HipRenderer, so the session composes them here."""
    import importlib
    fused = importlib.import_module("volume-rendering_amd.fusion").FusedRenderer
    tf2d = importlib.import_module("volume-rendering_amd.tf2d").Tf2dRenderer
    return type("SessionRenderer", (fused, tf2d), {})(device)


def _device_array(a):
    import torch
    a = np.array(a)                                      # (a writable copy: the pool's arrays are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def run_setter(vr, gpu, model, step):
    """the call of a setter step on the context, the values taken from the model AFTER model.apply(step); returns the status"""
    op, a, m = step.op, step.args, model
    try:
        if op == "set_window":
            gpu.set_window_buffer(a["w"], a["h"])
        elif op == "set_volume":
            gpu.set_volume(m.world.volume(a["key"]).data)
        elif op == "set_volume_device":
            import torch
            vox = m.world.volume(a["key"]).data
            t = _device_array(vox)
            torch.cuda.synchronize()
            gpu.set_volume_device(t.data_ptr(), vox.shape[::-1], vox.dtype.itemsize)
        elif op == "generate_volume":
            gpu.generate_volume(a["kind"], a["n"], seed=a["seed"], bytes_per_voxel=a["bpv"])
        elif op == "set_transfer_fn":
            gpu.set_transfer_fn(*m.tf.data)
        elif op == "set_clip":
            if a["name"] is None:
                gpu.clear_clip()
            else:
                box_min, box_max, plane = CLIPS[a["name"]]
                gpu.set_clip(box_min=box_min, box_max=box_max, plane=plane)
        elif op == "set_lighting":
            gpu.clear_lighting() if a["i"] is None else gpu.set_lighting(*LIGHTING_POOL[a["i"]])
        elif op == "set_shadow":
            if a["i"] is None:
                gpu.clear_shadow()
            else:
                light, S, shadow_step, strength, sampling = SHADOW_POOL[a["i"]]
                gpu.set_shadow(light, S, shadow_step, strength, CUTOFF, sampling)
        elif op == "set_preintegration":
            gpu.set_preintegration(a["on"])
        elif op in ("set_labels", "set_labels_device"):
            if a["salt"] is None:
                gpu.clear_labels()
            else:
                lab = m.world.labels(m.volume, a["salt"]).data
                if op == "set_labels":
                    gpu.set_labels(lab)
                else:
                    import torch
                    t = _device_array(lab)
                    torch.cuda.synchronize()
                    gpu.set_labels(t)
                    torch.cuda.synchronize()             # (the copy runs on the context's stream; the call has waited for it: t may go)
        elif op == "set_label_table":
            gpu.set_label_table(None if a["name"] is None else [tuple(float(v) for v in row) for row in m.world.label_tables[a["name"]]])
        elif op == "set_tf2d":
            if a["base"] is None:
                gpu.clear_tf2d()
            else:
                table, g_scale, bits = m.world.tf2d(m.volume, a["base"], a["g"]).data
                gpu.set_tf2d(table, g_scale, bits)
        elif op in ("set_second_volume", "set_second_volume_device"):
            if a["variant"] is None:
                gpu.clear_second_volume()
            else:
                b = m.world.second(m.volume, a["variant"]).data
                if op == "set_second_volume":
                    gpu.set_second_volume(b)
                else:
                    import torch
                    t = _device_array(b)
                    torch.cuda.synchronize()
                    gpu.set_second_volume(t)
                    torch.cuda.synchronize()
        elif op == "set_second_transfer_fn":
            gpu.set_second_transfer_fn(*m.second_tf.data)
        elif op == "refuse_second_copy":
            if a["on"]:
                os.environ["VR_SECOND_COPY_REFUSE"] = "1"
            else:
                os.environ.pop("VR_SECOND_COPY_REFUSE", None)
        elif op == "prepare":
            gpu.prepare()
        elif op == "release_linear_copy":
            gpu.release_linear_copy()
        elif op == "download_shadow":
            got = gpu.download_shadow()
            light, S, shadow_step, _, sampling = m.shadow.data
            want = ShadowRef.instance().build(light, S, shadow_step, m.volume.data, m.tf.data[0], CUTOFF, sampling, clip=m.clip.data if m.clip else None)
            assert np.array_equal(got, want), ("the light grid", int((got != want).sum()))
        elif op == "set_layout":
            gpu.set_layout(a["v"])
        elif op == "set_wide_addressing":
            gpu.set_wide_addressing(a["v"])
        elif op == "set_brick_plane":
            gpu.set_brick_plane(a["v"])
        elif op == "set_column_copy":
            gpu.set_column_copy(a["v"])
        elif op == "set_run_flavour":
            gpu.set_run_flavour(a["v"])
        elif op == "set_tile_scheduling":
            gpu.set_tile_scheduling(a["v"])
        elif op == "set_tile_mapping":
            gpu.set_tile_mapping(a["lane_map"], a["px"], a["py"])
        else:
            raise ValueError(op)
    except vr.VrError as e:
        return e.code
    return OK


def run_frame(vr, gpu, model, f, stream=None):
    """One frame step on the context through the host or the device entry point; returns a Want of what came back.  stream: a torch stream
    for the device entry point (None: torch's current one); the buffers are filled with 0x77 first so that an unwritten pixel shows."""
    w = model.world
    p = w.params(model.volume, f.view, f.sampling, f.march)
    k, device = f.kind, f.entry == "device"
    try:
        if k == "pick":
            got = gpu.pick(p, PICKS, f.opacity, f.mode)
            picks = np.zeros((len(PICKS), 10), np.float32)
            for i, g in enumerate(got):
                picks[i] = (float(g["hit"]), g["k"], g["value"], g["alpha"]) + tuple(g["position"]) + tuple(g["voxel"])
            return Want(picks=picks)
        if not device:
            if k == "volume":
                return Want(rgba=gpu.render_volume(p))
            if k == "mip":
                return Want(rgba=gpu.render_mip(p))
            if k == "iso":
                rgba, depth = gpu.render_iso(p, w.level(model.volume), f.refine, depth=True)
                return Want(rgba=rgba, depth=depth)
            if k == "backdrop":
                rgba, depth = layer_of(model, f)
                return Want(rgba=gpu.render_backdrop(p, rgba, depth))
            if k == "hybrid":
                rgba, depth = gpu.render_hybrid(p, w.level(model.volume), f.refine, depth=True)
                return Want(rgba=rgba, depth=depth)
            if k in ("section", "section_in_volume"):
                plane, half_width, mode, window = SECTIONS[f.section]
                call = gpu.render_section if k == "section" else gpu.render_section_in_volume
                rgba, depth = call(p, plane, half_width, mode, w.window_of(model.volume, window), depth=True)
                return Want(rgba=rgba, depth=depth)
            if k == "depth":
                depth, value, alpha = gpu.render_depth(p, f.opacity, f.mode, value=True, alpha=True)
                return Want(depth=depth, value=value, alpha=alpha)
            if k == "labelled":
                return Want(rgba=gpu.render_labelled(p))
            if k == "tf2d":
                return Want(rgba=gpu.render_tf2d(p))
            if k == "fused":
                return Want(rgba=gpu.render_fused(p, f.wa, f.wb, f.mode))
            raise ValueError(k)
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        with torch.cuda.stream(s):
            rgba = torch.full((p.out_rows, p.out_width, 4), 0x77, dtype=torch.uint8, device="cuda")
            floats = [torch.full((p.out_rows, p.out_width), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
            raw = s.cuda_stream
            own_depth = bool(f.args.get("own_depth"))
            out = {"rgba": rgba}
            if k == "volume":
                gpu.render_volume_device(p, rgba.data_ptr(), raw)
            elif k == "mip":
                gpu.render_mip_device(p, rgba.data_ptr(), raw)
            elif k == "iso":
                gpu.render_iso_device(p, w.level(model.volume), f.refine, rgba.data_ptr(), floats[0].data_ptr(), raw)
                out["depth"] = floats[0]
            elif k == "backdrop":
                layer_rgba, layer_depth = (torch.from_numpy(np.array(a)).cuda() for a in layer_of(model, f))
                gpu.render_backdrop_device(p, layer_rgba.data_ptr(), layer_depth.data_ptr(), rgba.data_ptr(), raw)
            elif k == "hybrid":
                gpu.render_hybrid_device(p, w.level(model.volume), f.refine, rgba.data_ptr(), None if own_depth else floats[0].data_ptr(), raw)
                if not own_depth:
                    out["depth"] = floats[0]
            elif k in ("section", "section_in_volume"):
                plane, half_width, mode, window = SECTIONS[f.section]
                call = gpu.render_section_device if k == "section" else gpu.render_section_in_volume_device
                keep = k == "section" or not own_depth
                call(p, plane, half_width, mode, w.window_of(model.volume, window), rgba.data_ptr(), floats[0].data_ptr() if keep else None, raw)
                if keep:
                    out["depth"] = floats[0]
            elif k == "depth":
                del out["rgba"]
                gpu.render_depth_device(p, f.opacity, f.mode, floats[0].data_ptr(), floats[1].data_ptr(), floats[2].data_ptr(), raw)
                out.update(depth=floats[0], value=floats[1], alpha=floats[2])
            elif k == "labelled":
                gpu.render_labelled_device(p, rgba.data_ptr(), raw)
            elif k == "tf2d":
                gpu.render_tf2d_device(p, rgba.data_ptr(), raw)
            elif k == "fused":
                gpu.render_fused_device(p, rgba.data_ptr(), raw, f.wa, f.wb, f.mode)
            else:
                raise ValueError(k)
        if stream is not None:
            return out                                   # queued: the caller synchronises and reads the tensors
        torch.cuda.synchronize()
        return Want(**{name: t.cpu().numpy() for name, t in out.items()})
    except vr.VrError as e:
        return Want(e.code)


def shown(want, got):
    """want restricted to the buffers that came back (a device frame with a context-owned depth hands none out)"""
    return Want(want.status, want.refusal, **{n: b for n, b in want.buffers.items() if n in got.buffers}) if want.status == OK and got.status == OK else want


CANONICAL = ("volume", "tf", "clip", "lighting", "shadow", "preint", "labels", "label_table", "tf2d", "second", "second_tf")


def fresh_verdict(vr, model, f, want):
    """The same frame once more on a fresh context given only the model's current state, in canonical order: "history" if that one matches
    the restatement — the session's context carried something its calls left behind —, "kernel/restatement" if it does not."""
    gpu = session_renderer(0)
    try:
        m = model
        gpu.set_window_buffer(*(m.window or SIZE))
        gpu.set_layout(m.knobs["layout"])
        gpu.set_wide_addressing(m.knobs["wide"])
        gpu.set_brick_plane(m.knobs["plane"])
        gpu.set_column_copy(m.knobs["column_copy"])
        gpu.set_run_flavour(m.knobs["run_flavour"])
        gpu.set_tile_mapping(*m.knobs["mapping"])
        gpu.set_tile_scheduling(m.knobs["scheduling"])
        gpu.set_volume(m.volume.data)
        gpu.set_transfer_fn(*m.tf.data)
        if m.clip:
            gpu.set_clip(box_min=m.clip.data[0], box_max=m.clip.data[1], plane=m.clip.data[2])
        if m.lighting:
            gpu.set_lighting(*m.lighting.data)
        if m.shadow:
            light, S, shadow_step, strength, sampling = m.shadow.data
            gpu.set_shadow(light, S, shadow_step, strength, CUTOFF, sampling)
        if m.preint:
            gpu.set_preintegration(1)
        if m.labels:
            gpu.set_labels(m.labels.data)
        if m.label_table:
            gpu.set_label_table([tuple(float(v) for v in row) for row in m.label_table.data])
        if m.tf2d:
            gpu.set_tf2d(*m.tf2d.data)
        if m.second:
            gpu.set_second_volume(m.second.data)
        if m.second_tf:
            gpu.set_second_transfer_fn(*m.second_tf.data)
        got = run_frame(vr, gpu, m, f)
        return "history" if shown(want, got).differs(got) == 0 else "kernel/restatement"
    finally:
        gpu.close()
