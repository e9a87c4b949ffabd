"""CPU tier of the session tests: the sequences of tests/session_helpers.py are worth running.  No GPU is used — the restatements alone
say what every frame of every sequence must be — and what is shown here is what gives tests/test_gpu_session.py its meaning:
(a) every pair of a state component and a frame kind that reads it (session_helpers.READS, read off include/vr_hip.h) is reached by a frame
    that follows a change of that component, and a stale value WOULD show there: the restatement under the component's previous value
    differs in at least 20 pixels (the per-frame floor of the random tiers), for a pick in at least one answer;
(b) every transition the invalidation rules of vr_hip_api.cpp exist for occurs and is followed by a frame that reads the component, and
    every documented refusal is predicted, between two successful frames of another kind;
(c) the model's drop and survive rules are the header's: each is held against the header's own words;
(d) a drop rule stated wrongly changes the expectation of some frame of the sequences — the GPU comparison would catch the same mistake
    made on the device side."""
import os
import re

import pytest

import feature_random as fr
import session_helpers as sh
from gpu_feature import PLANES, SCHEDULINGS, WIDES
from helpers import ROOT

FLOOR = 20                                              # test_gpu_feature_random.py: pixels > 20 * frames


@pytest.fixture(scope="module")
def world(vr, oracle):
    return sh.World.instance(vr, oracle)


@pytest.fixture(scope="module")
def walked(world):
    """name -> [(index, step, a copy of the model the step sees, promised status)]: frames see the state before them, setters the state they leave"""
    return {name: [(i, step, model.fork(), status) for i, step, model, status in sh.walk(world, steps)] for name, steps in sh.sequences(world).items()}


def test_the_sequences_are_deterministic_and_of_the_size_the_budget_allows(world):
    """the same lists on every call and from a writer of its own; 130 to 250 steps each, one line per step; five sequences, general0 the shortest
    general one; every frame is 48 x 40 from the three EDGE_VIEWS, through both entry points"""
    lists = sh.sequences(world)
    assert tuple(lists) == sh.NAMES == ("general0", "general1", "general2", "release", "refuse")
    for name, steps in lists.items():
        assert 130 <= len(steps) <= 250, (name, len(steps))
        again = sh._sequences.pop(name)
        assert [s.line() for s in sh.sequence(world, name)] == [s.line() for s in again], name
        assert all("\n" not in s.line() for s in steps)
        frames = [s for s in steps if s.is_frame]
        assert {f.view for f in frames} == set(fr.EDGE_VIEWS) and {f.entry for f in frames} == {"host", "device"}, name
        print(f"{name}: {len(steps)} steps, {len(frames)} frames")
    assert len(lists["general0"]) == min(len(lists[n]) for n in ("general0", "general1", "general2"))
    assert {s.op for steps in lists.values() for s in steps} >= {
        "set_window", "set_volume", "set_volume_device", "generate_volume", "set_transfer_fn", "set_clip", "set_lighting", "set_shadow", "set_preintegration",
        "set_labels", "set_labels_device", "set_label_table", "set_tf2d", "set_second_volume", "set_second_volume_device", "set_second_transfer_fn", "prepare",
        "release_linear_copy", "refuse_second_copy", "download_shadow", "set_layout", "set_wide_addressing", "set_brick_plane", "set_column_copy",
        "set_run_flavour", "set_tile_mapping", "set_tile_scheduling", "frame"}
    assert {f.kind for steps in lists.values() for f in steps if f.is_frame} == set(sh.KINDS)
    assert sh.trace(lists["general0"], 2).count("\n") == 2


def test_every_pair_is_reached_and_a_stale_value_would_show(world, walked):
    """(a): for every (component, kind) of READS the frame after a change of the component that tells its previous value from its current
    one best; none may be absent, none below the floor"""
    best = {}
    for name, steps in walked.items():
        for i, f, model, status in steps:
            if not f.is_frame or status != sh.OK:
                continue
            want = None
            for component in sh.READS:
                pair = (component, f.kind)
                floor = 1 if f.kind == "pick" else FLOOR
                if f.kind not in sh.READS[component] or model.changed[component] is None or best.get(pair, (0,))[0] >= 4 * floor:
                    continue
                stale = model.fork(component)
                if stale.volume is None or stale.tf is None or stale.refusal(f)[0] != sh.OK:
                    continue                            # (the previous value was "not set": a stale one would be a frame where a refusal is due)
                if component == "volume" and any(stale.now[c] is not None and stale.now[c].data.shape != stale.volume.data.shape for c in ("labels", "second")
                                                 if f.kind == sh.READER_OF[c]):
                    continue                            # (labels or B of other dims than the previous volume: no such state exists)
                want = sh.expected(model, f) if want is None else want
                differs = want.differs(sh.expected(stale, f))
                if differs > best.get(pair, (0,))[0]:
                    best[pair] = (differs, name, model.changed[component], i)
    print(f"{'component':12s} {'kind':18s} {'differs':>7s}  sequence  changed at  frame at")
    for component, kind in sh.PAIRS:
        differs, name, changed, i = best.get((component, kind), (0, "-", -1, -1))
        print(f"{component:12s} {kind:18s} {differs:7d}  {name:9s} {changed:10d} {i:9d}")
    missing = [pair for pair in sh.PAIRS if best.get(pair, (0,))[0] < (1 if pair[1] == "pick" else FLOOR)]
    assert len(sh.PAIRS) == 60 and not missing, missing


def test_transitions_and_refusals_are_covered(world, walked):
    """(b)"""
    every = [entry for steps in walked.values() for entry in steps]
    # set -> clear -> set, each followed by a frame that reads the component before the next change of it
    for component in ("clip", "lighting", "shadow", "preint", "labels", "tf2d", "second"):
        found = False
        for steps in walked.values():
            history = []                                # (set?, read?) per change of the component
            for i, step, model, status in steps:
                if not step.is_frame and model.changed[component] == i and status == sh.OK:
                    history.append([model.now[component] is not None, False])
                elif step.is_frame and history and step.kind in sh.READS[component]:
                    history[-1][1] = True
            states = [s for s, read in history if read]
            found = found or any(states[j:j + 3] == [True, False, True] for j in range(len(states)))
        assert found, component
    # the three kinds of volume change while labels, B, a 2-D table and a shadow are in place, and a reader of each behind it
    kinds = set()
    for steps in walked.values():
        for n, (i, step, model, status) in enumerate(steps):
            if step.op not in ("set_volume", "set_volume_device", "generate_volume") or n == 0:
                continue
            before = steps[n - 1][2]
            if any(before.now[c] is None for c in ("volume", "labels", "second", "tf2d", "shadow")):
                continue
            old, new = before.volume.data, model.volume.data
            kind = "voxel size" if old.dtype != new.dtype else ("contents" if old.shape == new.shape else "dims")
            readers = {s.kind for _, s, m, _ in steps[n + 1:n + 8] if s.is_frame and m.changed["volume"] == i}
            if {"labelled", "fused", "tf2d", "volume"} <= readers:
                kinds.add(kind)
    assert kinds == {"contents", "dims", "voxel size"}, kinds
    # a window grow between two host frames with depth
    for kind in ("iso", "hybrid", "depth"):
        assert any(a[1].is_frame and a[1].kind == kind and a[1].entry == "host" and b[1].op == "set_window" and c[1].is_frame and c[1].kind == kind and
                   c[1].entry == "host" and b[2].window[0] * b[2].window[1] > a[2].window[0] * a[2].window[1]
                   for steps in walked.values() for a, b, c in zip(steps, steps[1:], steps[2:])), kind
    # every knob value, a frame behind each
    for op, values in (("set_brick_plane", PLANES), ("set_wide_addressing", WIDES), ("set_tile_scheduling", SCHEDULINGS), ("set_layout", (0, 1)),
                       ("set_column_copy", (0, 1, 2)), ("set_run_flavour", (0, 1, 2))):
        seen = {a[1].v for steps in walked.values() for a, b in zip(steps, steps[1:]) if a[1].op == op and a[3] == sh.OK and b[1].is_frame and b[3] == sh.OK}
        assert seen == set(values), (op, seen)
    # every refusal, and behind it a successful frame of another kind that is the step in front of it: its expectation is unchanged
    seen = set()
    for steps in walked.values():
        for a, b, c in zip(steps, steps[1:], steps[2:]):
            if b[1].is_frame and b[3] != sh.OK and a[1].is_frame and c[1].is_frame and a[3] == c[3] == sh.OK and a[1].line() == c[1].line() and a[1].kind != b[1].kind:
                seen.add(b[2].refusal(b[1])[1])
                assert sh.expected(a[2], a[1]).differs(sh.expected(c[2], c[1])) == 0
    assert seen == set(sh.REFUSALS), set(sh.REFUSALS) ^ seen
    # the release: its refusals until the next set_volume; the refused copy of B: holds until B is set again, then clears
    release = walked["release"]
    promised = [(step.op, status) for _, step, _, status in release if not step.is_frame]
    assert ("release_linear_copy", sh.INVALID) in promised and ("release_linear_copy", sh.OK) in promised
    assert ("set_layout", sh.NOT_READY) in promised and ("set_wide_addressing", sh.NOT_READY) in promised
    released = [(i, step) for i, step, model, status in release if step.is_frame and model.released and status == sh.OK]
    assert {f.kind for _, f in released} == set(sh.KINDS) and any(f.kind == "mip" and f.march == "default" for _, f in released)
    layouts = [model.fused_layout(step) for _, step, model, status in walked["refuse"] if step.is_frame and step.kind == "fused" and status == sh.OK]
    compact = [x for j, x in enumerate(layouts) if x is not None and (j == 0 or x != layouts[j - 1])]
    assert compact[:3] == ["bricks", "linear", "bricks"] and layouts.count("linear") >= 6, compact
    every_frame = [e for e in every if e[1].is_frame]
    print(f"{len(every)} steps, {len(every_frame)} frames, {sum(e[3] != sh.OK for e in every_frame)} of them refused")


def _header():
    with open(os.path.join(ROOT, "include", "vr_hip.h")) as f:
        return re.sub(r"\s+", " ", f.read().replace(" * ", " "))


# (c): after X, is Y still set?  (the setters in order, the component asked about, is it set afterwards, the header's words)
FACTS = (
    (("labels", "volume"), "labels", False, "vr_hip_set_volume*, vr_hip_generate_volume drop them too: vr_hip_render_labelled* then returns VR_ERR_NOT_READY"),
    (("labels", "generate"), "labels", False, "vr_hip_set_volume*, vr_hip_generate_volume drop them too"),
    (("label_table", "volume"), "label_table", True, "The table survives until it is replaced"),
    (("label_table", "labels", "clear_labels"), "label_table", True, "The table survives until it is replaced"),
    (("second", "volume"), "second", False, "NULL drops B. vr_hip_set_volume*, vr_hip_generate_volume drop it too: vr_hip_render_fused* then returns VR_ERR_NOT_READY"),
    (("second", "second_tf", "volume"), "second_tf", True, "B's function and the bits survive a volume change until they are replaced"),
    (("second", "second_tf", "clear_second"), "second_tf", True, "B's function and the bits survive a volume change until they are replaced"),
    (("tf2d", "volume"), "tf2d", True, "The table is context state and is copied; NULL drops it. It survives a volume change"),
    (("tf2d", "tf"), "tf2d", True, "is independent of the 1-D transfer function"),
    (("clip", "shadow", "lighting", "preint", "volume"), "clip", True, "The clip is context state, like the layout knobs"),
    (("clip", "shadow", "lighting", "preint", "volume"), "shadow", True, "It is context state, like the clip: NULL switches it off, which is the default"),
    (("clip", "shadow", "lighting", "preint", "volume"), "lighting", True, "It is context state, like the clip and the shadow: NULL switches it off"),
    (("clip", "shadow", "lighting", "preint", "volume"), "preint", True, "It is context state, like the clip, the shadow and the lighting: off by default"),
    (("labels", "second", "tf"), "labels", True, "Setting labels or a table changes no other frame of the context: every other entry point ignores both"),
    (("labels", "second", "tf"), "second", True, "Every other entry point ignores all of this"),
)
_SETTERS = {"volume": sh.Step("set_volume", key="a2"), "generate": sh.Step("generate_volume", kind="noise", n=12, seed=3, bpv=1), "tf": sh.Step("set_transfer_fn", base=1),
            "labels": sh.Step("set_labels", salt=0), "clear_labels": sh.Step("set_labels", salt=None), "label_table": sh.Step("set_label_table", name="kinds"),
            "second": sh.Step("set_second_volume", variant="mirror_xz"), "clear_second": sh.Step("set_second_volume", variant=None),
            "second_tf": sh.Step("set_second_transfer_fn", which="hot"), "tf2d": sh.Step("set_tf2d", base=0, g=0), "clip": sh.Step("set_clip", name="box"),
            "shadow": sh.Step("set_shadow", i=0), "lighting": sh.Step("set_lighting", i=0), "preint": sh.Step("set_preintegration", on=1)}


@pytest.mark.parametrize("n", range(len(FACTS)))
def test_the_models_rules_are_the_headers(world, n):
    """(c): each fact of FACTS holds in the model, and its wording stands in include/vr_hip.h as quoted"""
    calls, component, still_set, words = FACTS[n]
    model = sh.SessionModel(world)
    for step in (sh.Step("set_window", w=48, h=40), sh.Step("set_volume", key="a"), sh.Step("set_transfer_fn", base=0)) + tuple(_SETTERS[c] for c in calls):
        assert model.apply(step) == sh.OK
    assert (model.now[component] is not None) == still_set, f"after {' -> '.join(calls)}: {component} {'stays' if still_set else 'goes'} — the header: \"{words}\""
    assert re.sub(r"\s+", " ", words) in _header(), f"include/vr_hip.h no longer says: \"{words}\""


def test_the_light_grid_goes_stale_as_the_header_says(world):
    """(c) for the one derived datum the ABI counts: "It goes stale on a vr_hip_set_shadow whose struct differs from the current one in more
    than `strength` ..., on vr_hip_set_volume* / vr_hip_generate_volume, on vr_hip_set_transfer_fn, and on a vr_hip_set_clip that differs
    from the current clip" — and an identical call of either, the lighting and the pre-integration leave it"""
    assert "a change of the strength alone keeps the grid" in _header() and "on vr_hip_set_transfer_fn, and on a vr_hip_set_clip that differs from the current clip" in _header()
    model = sh.SessionModel(world)
    for step in (sh.Step("set_window", w=48, h=40), sh.Step("set_volume", key="a"), sh.Step("set_transfer_fn", base=0)):
        model.apply(step)
    reader = sh.frame("volume")
    builds = []
    for step in (sh.Step("set_shadow", i=0), sh.Step("set_shadow", i=0), sh.Step("set_shadow", i=1), sh.Step("set_shadow", i=2), sh.Step("set_clip", name="box"),
                 sh.Step("set_clip", name="box"), sh.Step("set_clip", name=None), sh.Step("set_lighting", i=0), sh.Step("set_preintegration", on=1),
                 sh.Step("set_transfer_fn", base=0), sh.Step("set_volume", key="a2"), sh.Step("generate_volume", kind="noise", n=12, seed=3, bpv=1),
                 sh.Step("set_shadow", i=None), sh.Step("set_shadow", i=2)):
        model.apply(step)
        model.count(reader)
        builds.append(model.shadow_builds)
    assert builds == [1, 1, 1, 2, 3, 3, 4, 4, 4, 5, 6, 7, 7, 8], builds
    model.apply(sh.Step("set_transfer_fn", base=1))
    model.count(sh.frame("mip"))                        # no reader: the grid stays stale and nothing is built
    assert model.shadow_builds == 8 and model.shadow_stale


WRONG = ("labels survive a volume", "B survives a volume", "tf2d goes with the volume", "label table goes with the volume", "B's function goes with B")


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_drop_rule_changes_a_frame_of_the_sequences(world, walked, wrong):
    """(d): with one rule of the model wrong, some frame of the sequences is promised another status or other bytes"""
    found = []
    for name, steps in sh.sequences(world).items():
        for (i, f, right, status), (_, _, model, other) in zip(walked[name], sh.walk(world, steps, wrong)):
            if not f.is_frame:
                continue
            if status != other or (status == sh.OK and sh.expected(right, f).differs(sh.expected(model, f)) != 0):
                found.append((name, i, f.line(), status, other))
                break
    print(wrong, found)
    assert found, wrong
