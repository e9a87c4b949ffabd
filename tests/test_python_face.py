"""The Python face of the C ABI (volume-rendering_amd/renderer.py: HipRenderer, MultiRenderer), pinned on the CPU: the loader the two
classes call is replaced by a recorder, so every public method runs without libvr_hip.so.  Held against tests/golden/python_face.json:
the sequence of (entry, arguments) each call of a method makes — structs by their bytes (by member where they hold pointers), pointers
and addresses as null / non-null, ctypes arrays by type and bytes — the type, dtype and shape of what it returns, the exception of a run
in which one entry fails, every public signature, and the package's __all__.  Every case runs on a fresh renderer, the first case of every
render, pick and shadow method also after a set_shadow(step=None), whose pending step composite-type frames resolve and nothing else does.
`python tests/test_python_face.py --record` writes the fixture from the tree it is in."""
import ctypes as C
import importlib
import inspect
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "python_face.json")
vr = importlib.import_module("volume-rendering_amd")
face = importlib.import_module("volume-rendering_amd.renderer")

DEV, DEV2, DEV3, STREAM = 0x7f0000001000, 0x7f0000002000, 0x7f0000003000, 0x7f0000004000
PLANE = (0.0, 0.0, 1.0, 0.25)


def describe(a):
    """one argument of an entry, as the fixture holds it"""
    if a is None or isinstance(a, (bool, float, str)):
        return a
    if isinstance(a, int):
        return "non-null" if a >= 1 << 32 else a            # an address (of a numpy buffer, or one of DEV.. above) against a scalar
    if isinstance(a, bytes):
        return a.decode()
    if hasattr(a, "_obj"):                                  # byref(x)
        return ["byref", describe(a._obj)]
    if isinstance(a, vr.VrParams) and bytes(a) == bytes(params()):
        return "params()"
    if isinstance(a, C.Structure):
        if any(t is C.c_void_p for _, t in a._fields_):
            return [type(a).__name__, {n: ("non-null" if getattr(a, n) else "null") if t is C.c_void_p else describe(getattr(a, n)) for n, t in a._fields_}]
        return [type(a).__name__, bytes(a).hex()]
    if isinstance(a, C.Array):
        return [type(a).__name__, bytes(a).hex()]
    if isinstance(a, C.c_void_p):
        return "non-null" if a.value else "null"
    if isinstance(a, C._Pointer):
        return "non-null" if a else "null"
    if isinstance(a, C._SimpleCData):
        return [type(a).__name__, a.value]
    raise TypeError(f"an argument the recorder does not know: {type(a)}")


def describe_result(v):
    if isinstance(v, np.ndarray):
        return ["ndarray", str(v.dtype), list(v.shape)]
    if isinstance(v, (tuple, list)):
        return [type(v).__name__, [describe_result(x) for x in v]]
    if isinstance(v, dict):
        return ["dict", {k: describe_result(x) for k, x in v.items()}]
    if isinstance(v, C.Structure):
        return [type(v).__name__]
    return [type(v).__name__, v]


class Recorder:
    """stands in for the loaded library: every entry records its arguments and returns 0 — or 1, at the call numbered fail_at"""
    def __init__(self):
        self.calls, self.fail_at = [], None

    def __getattr__(self, name):
        if not name.startswith("vr_h"):
            raise AttributeError(name)
        return lambda *args: self.call(name, args)

    def call(self, name, args):
        index = len(self.calls)
        self.calls.append([name] + [describe(a) for a in args])
        if name in ("vr_hip_destroy", "vr_hip_multi_destroy"):
            return None
        if name in ("vr_hip_last_error", "vr_hip_multi_last_error"):
            return b"the recorder's error"
        if name == "vr_hip_multi_transport":
            return b"recorded"
        if name == "vr_hip_multi_context":
            return 0x7f0000005000
        if index == self.fail_at:
            return 1
        if name in ("vr_hip_create", "vr_hip_multi_create"):
            args[-1]._obj.value = 0x7f0000006000
        elif name == "vr_hip_download_shadow":
            args[3]._obj.value = 3
        elif name == "vr_hip_read_tile_costs":
            args[3]._obj.value, args[4]._obj.value = 3, 2
        elif name == "vr_hip_download_copy" and args[4] is not None:
            args[4]._obj.value = 40
        return 0


def params():
    p = vr.VrParams()
    p.view.width, p.view.height, p.view.perspective = 6, 4, 1
    p.ray_step, p.ray_threshold, p.light_kd, p.esl, p.esl_block_dims, p.sampling = 0.0625, 0.95, 0.5, 1, 4, vr.SAMPLE_TRILINEAR
    return vr.whole_frame(p)


class Tensor:
    """what set_labels asks of a device tensor"""
    def __init__(self, dtype="torch.uint8", shape=(2, 3, 4), contiguous=True, cuda=True):
        self.dtype, self.shape, self.contiguous, self.is_cuda = dtype, shape, contiguous, cuda

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self.contiguous

    def data_ptr(self):
        return DEV


def u8(*shape):
    return np.zeros(shape, np.uint8)


def f32(*shape):
    return np.zeros(shape, np.float32)


# every public method, with canned arguments: both branches of every optional argument
SINGLE = {
    "close": [lambda r: r.close(), lambda r: (r.close(), r.close())],
    "get_name": [lambda r: r.get_name()],
    "set_window_buffer": [lambda r: r.set_window_buffer(6, 4)],
    "set_transfer_fn": [lambda r: r.set_transfer_fn(f32(128, 4), np.zeros(1024, np.uint32)), lambda r: r.set_transfer_fn(f32(127, 4), np.zeros(1024, np.uint32)),
                        lambda r: r.set_transfer_fn(np.zeros((128, 4), np.float64), [0] * 1024)],
    "set_volume": [lambda r: (r.set_volume(u8(2, 3, 4)), r.dims, r.bytes_per_voxel), lambda r: (r.set_volume(np.zeros((2, 3, 4), np.uint16)), r.dims, r.bytes_per_voxel),
                   lambda r: r.set_volume(f32(2, 3, 4)), lambda r: r.set_volume(u8(3, 4))],
    "set_volume_device": [lambda r: (r.set_volume_device(DEV, [4, 3, 2], 2), r.dims, r.bytes_per_voxel)],
    "set_layout": [lambda r: r.set_layout(vr.LAYOUT_BRICKED)],
    "set_wide_addressing": [lambda r: r.set_wide_addressing(2), lambda r: r.set_wide_addressing(False)],
    "set_brick_plane": [lambda r: r.set_brick_plane(), lambda r: r.set_brick_plane(2)],
    "set_column_copy": [lambda r: r.set_column_copy(), lambda r: r.set_column_copy(2)],
    "set_run_flavour": [lambda r: r.set_run_flavour(), lambda r: r.set_run_flavour(vr.RUN_FLAVOUR_SEVEN)],
    "run_aligned_info": [lambda r: r.run_aligned_info()],
    "set_tile_mapping": [lambda r: r.set_tile_mapping(), lambda r: r.set_tile_mapping(1, 2, 3)],
    "set_tile_scheduling": [lambda r: r.set_tile_scheduling(), lambda r: r.set_tile_scheduling(0)],
    "set_clip": [lambda r: r.set_clip(), lambda r: r.set_clip((-0.5, -0.25, -1), (0.5, 1, 0.75), (0, 1, 0, 0.125)), lambda r: r.set_clip(plane=(1, 0, 0, 0))],
    "clear_clip": [lambda r: r.clear_clip()],
    "set_shadow": [lambda r: (r.set_shadow((1, 2, 3)), r._shadow), lambda r: (r.set_shadow((1, 2, 3), 64, 0.02, 0.5, 0.01, 2), r._shadow),
                   lambda r: (r.set_shadow((1, 2, 3), dims=32, strength=0.25), r.render_volume(params()), r.render_volume(params()), r._shadow)],
    "clear_shadow": [lambda r: (r.clear_shadow(), r._shadow)],
    "download_shadow": [lambda r: r.download_shadow(), lambda r: r.download_shadow(0.03125), lambda r: r.download_shadow(ray_step=0.03125)],
    "shadow_builds": [lambda r: r.shadow_builds()],
    "set_lighting": [lambda r: r.set_lighting(), lambda r: r.set_lighting(0.1, 0.2, 0.3, 7), lambda r: r.set_lighting(shininess_log2=-1)],
    "clear_lighting": [lambda r: r.clear_lighting()],
    "lighting_frames": [lambda r: r.lighting_frames()],
    "set_preintegration": [lambda r: r.set_preintegration(), lambda r: r.set_preintegration(False), lambda r: r.set_preintegration(2)],
    "clear_preintegration": [lambda r: r.clear_preintegration()],
    "preint_frames": [lambda r: r.preint_frames()],
    "download_tf_integral": [lambda r: r.download_tf_integral()],
    "last_launch": [lambda r: r.last_launch()],
    "tile_costs": [lambda r: r.tile_costs()],
    "generate_volume": [lambda r: (r.generate_volume("shell", 8), r.dims, r.bytes_per_voxel), lambda r: (r.generate_volume("noise", 8, 3, 2), r.dims, r.bytes_per_voxel),
                        lambda r: r.generate_volume("bogus", 8)],
    "download_volume": [lambda r: (r.set_volume(u8(2, 3, 4)), r.download_volume()), lambda r: (r.set_volume_device(DEV, (4, 3, 2), 2), r.download_volume())],
    "render_volume": [lambda r: r.render_volume(params())],
    "render_volume_device": [lambda r: r.render_volume_device(params(), DEV), lambda r: r.render_volume_device(params(), DEV, STREAM), lambda r: r.render_volume_device(params(), DEV, stream=0)],
    "render_mip": [lambda r: r.render_mip(params())],
    "render_mip_device": [lambda r: r.render_mip_device(params(), DEV), lambda r: r.render_mip_device(params(), DEV, stream=STREAM)],
    "render_iso": [lambda r: r.render_iso(params(), 100), lambda r: r.render_iso(params(), 77.5, 9, depth=True), lambda r: r.render_iso(params(), 100, refine=0, depth=False)],
    "render_iso_device": [lambda r: r.render_iso_device(params(), 100, 4, DEV), lambda r: r.render_iso_device(params(), 100, 4, DEV, DEV2, STREAM),
                          lambda r: r.render_iso_device(params(), 100, 4, DEV, depth_ptr=0, stream=STREAM)],
    "render_backdrop": [lambda r: r.render_backdrop(params(), u8(4, 6, 4), f32(4, 6)), lambda r: r.render_backdrop(params(), u8(4, 6, 3), f32(4, 6)),
                        lambda r: r.render_backdrop(params(), u8(4, 6, 4), f32(4, 5)), lambda r: r.render_backdrop(params(), np.zeros((4, 6, 4), np.int64), np.zeros((4, 6), np.float64))],
    "render_backdrop_device": [lambda r: r.render_backdrop_device(params(), DEV, DEV2, DEV3), lambda r: r.render_backdrop_device(params(), 0, 0, DEV, stream=STREAM),
                               lambda r: r.render_backdrop_device(params(), DEV, DEV2, DEV, STREAM)],
    "render_hybrid": [lambda r: r.render_hybrid(params(), 100), lambda r: r.render_hybrid(params(), 77.5, 9, depth=True)],
    "render_hybrid_device": [lambda r: r.render_hybrid_device(params(), 100, 4, DEV), lambda r: r.render_hybrid_device(params(), 100, 4, DEV, DEV2, STREAM),
                             lambda r: r.render_hybrid_device(params(), 100, 4, DEV, depth_ptr=DEV2)],
    "backdrop_frames": [lambda r: r.backdrop_frames()],
    "render_section": [lambda r: r.render_section(params(), PLANE), lambda r: r.render_section(params(), PLANE, 0.125, "mean", (10, 200), depth=True),
                       lambda r: r.render_section(params(), PLANE, 0.125, 2, window=None), lambda r: r.render_section(params(), PLANE, mode="bogus")],
    "render_section_device": [lambda r: r.render_section_device(params(), PLANE, 0.0, "point", None, DEV),
                              lambda r: r.render_section_device(params(), PLANE, 0.125, "max", (10, 200), DEV, DEV2, STREAM),
                              lambda r: r.render_section_device(params(), PLANE, 0.125, "min", None, DEV, stream=STREAM)],
    "render_section_in_volume": [lambda r: r.render_section_in_volume(params(), PLANE), lambda r: r.render_section_in_volume(params(), PLANE, 0.125, "mean", (10, 200), depth=True),
                                 lambda r: r.render_section_in_volume(params(), PLANE, 0.125, 1, window=None)],
    "render_section_in_volume_device": [lambda r: r.render_section_in_volume_device(params(), PLANE, 0.0, "point", None, DEV),
                                        lambda r: r.render_section_in_volume_device(params(), PLANE, 0.125, "max", (10, 200), DEV, DEV2, STREAM),
                                        lambda r: r.render_section_in_volume_device(params(), PLANE, 0.125, "min", None, DEV, depth_ptr=DEV2)],
    "section_frames": [lambda r: r.section_frames()],
    "render_depth": [lambda r: r.render_depth(params(), 0.5), lambda r: r.render_depth(params(), 0.375, "peak", value=True), lambda r: r.render_depth(params(), 0.375, "mean", alpha=True),
                     lambda r: r.render_depth(params(), 0.375, 2, True, True), lambda r: r.render_depth(params(), 0.5, "bogus")],
    "render_depth_device": [lambda r: r.render_depth_device(params(), 0.5, "first", DEV), lambda r: r.render_depth_device(params(), 0.375, "mean", DEV, DEV2, DEV3, STREAM),
                            lambda r: r.render_depth_device(params(), 0.375, 1, DEV, alpha_ptr=DEV3), lambda r: r.render_depth_device(params(), 0.375, 1, 0, value_ptr=DEV2)],
    "pick": [lambda r: r.pick(params(), [(1, 2), (3, 4)], 0.5), lambda r: r.pick(params(), [], 0.375, "peak"), lambda r: r.pick(params(), np.array([5, 3]), 0.5, mode=2),
             lambda r: r.pick(params(), [(-1, 2)], 0.5), lambda r: r.pick(params(), [(1, 1 << 32)], 0.5)],
    "depth_frames": [lambda r: r.depth_frames()],
    "set_labels": [lambda r: r.set_labels(u8(2, 3, 4)), lambda r: r.set_labels(np.zeros((2, 3, 4), np.uint16)), lambda r: r.set_labels(u8(3, 4)), lambda r: r.set_labels(Tensor()),
                   lambda r: r.set_labels(Tensor(dtype="torch.int8")), lambda r: r.set_labels(Tensor(shape=(3, 4))), lambda r: r.set_labels(Tensor(contiguous=False)),
                   lambda r: r.set_labels(Tensor(cuda=False))],
    "clear_labels": [lambda r: r.clear_labels()],
    "set_label_table": [lambda r: r.set_label_table(), lambda r: r.set_label_table([]),
                        lambda r: r.set_label_table([vr.VrLabelEntry((1.0, 0.5, 0.25), 0.5, 1.0), dict(colour=(0, 1, 0), mix=1.0, opacity=0.0), (0.25, 0.5, 0.75, 0.125, 0.875), {}]),
                        lambda r: r.set_label_table(iter([(1, 0, 0, 1, 1)]))],
    "render_labelled": [lambda r: r.render_labelled(params())],
    "render_labelled_device": [lambda r: r.render_labelled_device(params(), DEV), lambda r: r.render_labelled_device(params(), DEV, STREAM)],
    "labelled_frames": [lambda r: r.labelled_frames()],
    "timing": [lambda r: r.timing()],
    "timing_reset": [lambda r: r.timing_reset()],
    "volume_minmax": [lambda r: r.volume_minmax()],
    "volume_histogram": [lambda r: r.volume_histogram()],
    "volume_info": [lambda r: r.volume_info()],
    "prepare": [lambda r: r.prepare(), lambda r: r.prepare(vr.COPY_VOXEL | vr.COPY_RUN_Z)],
    "download_copy": [lambda r: r.download_copy(5)],
    "release_linear_copy": [lambda r: r.release_linear_copy()],
    "device_info": [lambda r: r.device_info()],
}
MULTI = {
    "close": [lambda r: r.close(), lambda r: (r.close(), r.close())],
    "set_window_buffer": [lambda r: r.set_window_buffer(6, 4)],
    "set_transfer_fn": [lambda r: r.set_transfer_fn(f32(128, 4), np.zeros(1024, np.uint32)), lambda r: r.set_transfer_fn(np.zeros((128, 4), np.float64), [0] * 1024)],
    "set_clip": [lambda r: r.set_clip(), lambda r: r.set_clip((-0.5, -0.25, -1), (0.5, 1, 0.75), (0, 1, 0, 0.125))],
    "clear_clip": [lambda r: r.clear_clip()],
    "set_shadow": [lambda r: (r.set_shadow((1, 2, 3)), r._shadow), lambda r: (r.set_shadow((1, 2, 3), 64, 0.02, 0.5, 0.01, 2), r._shadow),
                   lambda r: (r.set_shadow((1, 2, 3), dims=32, strength=0.25), r.render_volume(params()), r.render_volume(params()), r._shadow)],
    "clear_shadow": [lambda r: (r.clear_shadow(), r._shadow)],
    "set_lighting": [lambda r: r.set_lighting(), lambda r: r.set_lighting(0.1, 0.2, 0.3, 7)],
    "clear_lighting": [lambda r: r.clear_lighting()],
    "set_preintegration": [lambda r: r.set_preintegration(), lambda r: r.set_preintegration(False)],
    "set_volume": [lambda r: r.set_volume(u8(2, 3, 4)), lambda r: r.set_volume(np.zeros((2, 3, 4), np.uint16))],
    "generate_volume": [lambda r: r.generate_volume("shell", 8), lambda r: r.generate_volume("noise", 8, 3, 2)],
    "render_volume": [lambda r: r.render_volume(params())],
    "render_volume_device": [lambda r: r.render_volume_device(params(), DEV)],
    "render_volume_device_async": [lambda r: r.render_volume_device_async(params(), DEV), lambda r: r.render_volume_device_async(params(), DEV, STREAM),
                                   lambda r: r.render_volume_device_async(params(), DEV, consumer_stream=0)],
    "sync": [lambda r: r.sync()],
    "prepare": [lambda r: r.prepare(), lambda r: r.prepare(vr.COPY_VOXEL)],
    "context_timing": [lambda r: r.context_timing(1)],
    "timing": [lambda r: r.timing()],
    "transport": [lambda r: r.transport],                   # a property
}
CLASSES = {"HipRenderer": (vr.HipRenderer, SINGLE, lambda: vr.HipRenderer(1)), "MultiRenderer": (vr.MultiRenderer, MULTI, lambda: vr.MultiRenderer([0, 2]))}


def public_methods(cls):
    return {n: f for n, f in inspect.getmembers(cls, inspect.isfunction) if not n.startswith("_")}


def one_run(recorder, make, case, pending_shadow, fail_at=None):
    """a fresh renderer, optionally a set_shadow(step=None), then the case; -> (calls of the case, what it gave)"""
    del recorder.calls[:]
    recorder.fail_at = None
    r = make()
    if pending_shadow:
        r.set_shadow((3, 2, 1), 16)
    first = len(recorder.calls)
    recorder.fail_at = None if fail_at is None else first + fail_at
    try:
        got = ["returns", describe_result(case(r))]
    except vr.VrError as e:
        got = ["raises", "VrError", e.code, str(e)]
    except (ValueError, KeyError) as e:
        got = ["raises", type(e).__name__, str(e)]
    recorder.fail_at = None
    calls = recorder.calls[first:]
    r.close()
    return calls, got


def record(monkeypatch=None):
    recorder = Recorder()
    if monkeypatch is not None:
        monkeypatch.setattr(face, "lib", lambda: recorder)
    else:
        face.lib = lambda: recorder
    out = {"__all__": list(vr.__all__), "signatures": {}, "runs": {}, "construction": {}}
    for cls_name, (cls, cases, make) in CLASSES.items():
        methods = public_methods(cls)
        out["signatures"][cls_name] = {n: str(inspect.signature(f)) for n, f in sorted(methods.items())}
        properties = sorted(n for n, p in inspect.getmembers(cls, lambda p: isinstance(p, property)) if not n.startswith("_"))
        assert set(cases) == set(methods) | set(properties), sorted(set(cases) ^ (set(methods) | set(properties)))
        for name in sorted(cases):
            for i, case in enumerate(cases[name]):
                frame_or_shadow = any(word in name for word in ("render", "pick", "shadow"))
                for pending in (False, True)[:2 if i == 0 and frame_or_shadow else 1]:          # after a pending set_shadow: every such method once
                    calls, got = one_run(recorder, make, case, pending)
                    failing = []
                    for k, c in enumerate(calls if i == 0 and not pending else []):         # one entry failing: the first case of every method
                        if c[0] in ("vr_hip_destroy", "vr_hip_multi_destroy", "vr_hip_last_error", "vr_hip_multi_last_error", "vr_hip_multi_transport", "vr_hip_multi_context"):
                            continue
                        n_calls, what = one_run(recorder, make, case, pending, fail_at=k)
                        failing.append([k, len(n_calls)] + (what[3:] if what[:3] == ["raises", "VrError", 1] else what))      # the usual VrError(1): its text alone
                    out["runs"][f"{cls_name}.{name}#{i}{' after set_shadow(step=None)' if pending else ''}"] = {"calls": calls, "gives": got, "failing": failing}
        # construction: the calls of a good one, of one whose create fails without a handle and of one that fails with a handle; __del__ closes
        for label, code, handle in (("ok", 0, True), ("no device", 2, False), ("failed with a context", 4, True)):
            del recorder.calls[:]

            def create(name, args, code=code, handle=handle, plain=Recorder.call):
                if name in ("vr_hip_create", "vr_hip_multi_create"):
                    recorder.calls.append([name] + [describe(a) for a in args])
                    args[-1]._obj.value = 0x7f0000006000 if handle else None
                    return code
                return plain(recorder, name, args)
            recorder.call = create
            try:
                r = make()
                got = ["returns", sorted(k for k in vars(r) if not k.startswith("_L")), describe_result(getattr(r, "device", None)), describe_result(getattr(r, "devices", None))]
                del r
            except vr.VrError as e:
                got = ["raises", "VrError", e.code, str(e)]
            del recorder.call
            out["construction"][f"{cls_name}: {label}"] = {"calls": list(recorder.calls), "gives": got}
    return out


def test_python_face_holds_calls_results_errors_signatures_and_all(monkeypatch):
    got = json.loads(json.dumps(record(monkeypatch)))
    with open(FIXTURE) as f:
        want = json.load(f)
    assert got["__all__"] == want["__all__"]
    assert got["signatures"] == want["signatures"]
    assert got["construction"] == want["construction"]
    assert sorted(got["runs"]) == sorted(want["runs"])
    wrong = [k for k in got["runs"] if got["runs"][k] != want["runs"][k]]
    for k in wrong[:4]:
        print(k, "\n  got ", json.dumps(got["runs"][k]), "\n  want", json.dumps(want["runs"][k]))
    assert not wrong, (len(wrong), wrong[:12])
    assert len(got["signatures"]["HipRenderer"]) == 66 and len(got["signatures"]["MultiRenderer"]) == 19


def test_private_names_other_files_use_stay(monkeypatch):
    recorder = Recorder()
    monkeypatch.setattr(face, "lib", lambda: recorder)
    single, multi = vr.HipRenderer(0), vr.MultiRenderer([0])
    assert single._L is recorder and multi._L is recorder and single._ctx.value and multi._m.value
    assert single._shadow is None and multi._shadow is None
    assert callable(single._resolve_shadow) and callable(multi._resolve_shadow)


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        recorded = record()
        def compact(v):
            return json.dumps(v, separators=(",", ":"))
        runs = "{\n" + ",\n".join(f" {json.dumps(n)}: {compact(x)}" for n, x in recorded["runs"].items()) + "\n}"      # one run per line
        with open(FIXTURE, "w") as f:
            f.write("{" + ",\n".join(f"{json.dumps(k)}: {runs if k == 'runs' else compact(v)}" for k, v in recorded.items()) + "}\n")
        print(f"{len(recorded['runs'])} runs -> {FIXTURE}")
    else:
        sys.exit("usage: python tests/test_python_face.py --record")
