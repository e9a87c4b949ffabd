"""GPU tier of the session tests: a frame depends on the context's current state alone, not on the calls that led there.  One context is
driven through each sequence of tests/session_helpers.py in lockstep with the model; every frame — RGBA bytes, the bit patterns of depths,
values and alphas, picks field by field — and every refusal is held against what the restatements give for the model's current state, no
tolerance anywhere, and at the end the testing aids of the ABI must have counted what the model counted.  tests/test_session_model.py shows
on the CPU that a stale value of every component would change some frame compared here."""
import os

import pytest

import session_helpers as sh
from gpu_feature import needs_bounds_lib, run_under_bounds_build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(vr, oracle):
    return sh.World.instance(vr, oracle)


@pytest.fixture(scope="module")
def gpu(vr):
    """a renderer of this module's own with every frame kind, on cuda:0, closed at the end"""
    import torch  # noqa: F401  (loads the process's HIP runtime first)
    r = sh.session_renderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def aid_off_afterwards(monkeypatch):
    """the library's testing aid is process state: no test leaves it set"""
    monkeypatch.delenv("VR_SECOND_COPY_REFUSE", raising=False)
    yield
    os.environ.pop("VR_SECOND_COPY_REFUSE", None)


def counters(gpu):
    return {"lighting": gpu.lighting_frames(), "preint": gpu.preint_frames(), "backdrop": gpu.backdrop_frames(), "section": gpu.section_frames(),
            "depth": gpu.depth_frames(), "labelled": gpu.labelled_frames(), "tf2d": gpu.tf2d_frames(), "fused": gpu.fused_frames()}


@pytest.mark.parametrize("name", sh.NAMES)
def test_sessions_equal_the_restatements(vr, world, name):
    """One context of its own per sequence.  Every setter returns the status the header promises, every frame the promised status and the
    restatement's buffers; a fused frame reads both linear arrays exactly while B's copy is refused.  On the first mismatch the frame is
    rendered once more on a fresh context given only the model's current state — the verdict (`history`: the session's context carried
    something over; `kernel/restatement`: the frame is wrong from any history) goes into the message with the trace — and the test fails.
    After the last step the per-kind frame counters and the builds of the light grid equal the model's."""
    import torch  # noqa: F401
    steps = sh.sequence(world, name)
    gpu = sh.session_renderer(0)
    compared = 0
    try:
        for i, step, model, status in sh.walk(world, steps):
            if not step.is_frame:
                try:
                    got = sh.run_setter(vr, gpu, model, step)
                except AssertionError as e:             # (the light grid a download_shadow step hands out)
                    raise AssertionError(f"step {i}: {e}\n{sh.trace(steps, i)}")
                assert got == status, f"step {i} returned {got}, the header promises {status}\n{sh.trace(steps, i)}"
                continue
            want = sh.expected(model, step)
            got = sh.run_frame(vr, gpu, model, step)
            differs = sh.shown(want, got).differs(got)
            if differs != 0:
                verdict = sh.fresh_verdict(vr, model, step, want) if want.status == sh.OK else "status"
                info = gpu.last_launch()
                raise AssertionError(f"step {i}: {differs} elements differ (status {got.status}, promised {want.status}); verdict: {verdict}; {info}\n{sh.trace(steps, i)}")
            if status == sh.OK:
                compared += 1
                if step.kind == "fused":
                    held, layout = model.fused_layout(step), gpu.last_launch()["layout"]
                    assert held is None or (layout == 0) == (held == "linear"), f"step {i}: layout {layout}, B's copy {held}\n{sh.trace(steps, i)}"
        assert counters(gpu) == model.counts, (counters(gpu), model.counts)
        assert gpu.shadow_builds()[0] == model.shadow_builds, (gpu.shadow_builds(), model.shadow_builds)
        print(f"{name}: {len(steps)} steps, {compared} frames compared, {model.shadow_builds} builds of the light grid")
    finally:
        gpu.close()


# (the setter, the kind whose frames read what it rewrites): every setter that rewrites device memory a frame in flight may read
DRAINS = (("set_transfer_fn", "volume"), ("set_labels", "labelled"), ("set_label_table", "labelled"), ("set_tf2d", "tf2d"), ("set_second_volume", "fused"),
          ("set_second_transfer_fn", "fused"), ("set_volume", "volume"))


@pytest.mark.parametrize("setter,kind", DRAINS)
def test_setters_wait_for_frames_in_flight(vr, world, gpu, setter, kind):
    """"The call waits for the context's frames first": four device-entry frames of a kind that reads the component are queued on a torch
    side stream, the setter is called at once, then everything is synchronised.  All four buffers hold the frame of the state BEFORE the
    setter, and the next frame holds the state after it.  Nothing widens the window: the frames need not be in flight when the setter runs;
    the ordering contract is what is asserted."""
    import torch
    model = sh.SessionModel(world)
    prologue = [sh.Step("set_window", w=48, h=40), sh.Step("set_layout", v=1), sh.Step("set_volume", key="ragged"), sh.Step("set_transfer_fn", base=0),
                sh.Step("set_clip", name=None), sh.Step("set_lighting", i=None), sh.Step("set_shadow", i=None), sh.Step("set_preintegration", on=0),
                sh.Step("set_labels", salt=0), sh.Step("set_label_table", name="kinds"), sh.Step("set_tf2d", base=0, g=0), sh.Step("set_second_volume", variant="mirror_xz"),
                sh.Step("set_second_transfer_fn", which="hot")]
    for step in prologue:
        assert model.apply(step) == sh.OK and sh.run_setter(vr, gpu, model, step) == sh.OK, step
    change = {"set_transfer_fn": sh.Step("set_transfer_fn", base=1), "set_labels": sh.Step("set_labels", salt=1), "set_label_table": sh.Step("set_label_table", name="faded"),
              "set_tf2d": sh.Step("set_tf2d", base=1, g=1), "set_second_volume": sh.Step("set_second_volume", variant="mirror_y"),
              "set_second_transfer_fn": sh.Step("set_second_transfer_fn", which="open"), "set_volume": sh.Step("set_volume", key="a")}[setter]
    f = sh.frame(kind, view=1, sampling=1, march="full", entry="device", mode="over", wa=1.0, wb=1.0)
    before = sh.expected(model, f)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    queued = [sh.run_frame(vr, gpu, model, f, stream=side) for _ in range(4)]
    assert all(isinstance(q, dict) for q in queued), queued
    after_model = model.fork()
    assert after_model.apply(change) == sh.OK
    assert sh.run_setter(vr, gpu, after_model, change) == sh.OK
    torch.cuda.synchronize()
    for n, q in enumerate(queued):
        got = sh.Want(rgba=q["rgba"].cpu().numpy())
        assert before.differs(got) == 0, (setter, "frame", n, "queued before the setter", before.differs(got))
    if setter == "set_volume":                          # (the new volume has dropped nothing this kind needs; its frame is the new volume's)
        assert after_model.labels is None and after_model.second is None
    host = sh.frame(kind, view=1, sampling=1, march="full", entry="host", mode="over", wa=1.0, wb=1.0)
    after = sh.expected(after_model, host)
    assert after.status == sh.OK and before.differs(after) >= 20, (setter, "the setter must show")
    got = sh.run_frame(vr, gpu, after_model, host)
    assert after.differs(got) == 0, (setter, "the frame behind the setter", after.differs(got))


@needs_bounds_lib
def test_sessions_under_the_bounds_checked_build():
    """The shortest general sequence and the release sequence once in a child process with the -DVR_BOUNDS_CHECK library
    (tests/test_gpu_bounds.py): every gather address of every frame of a session is held against its array — a violation fails the call"""
    run_under_bounds_build(__file__, "sessions_equal and (general0 or release)", 2, timeout=900)
