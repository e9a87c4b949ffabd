#!/usr/bin/env python3
"""Generates tests/golden/ from the REFERENCE'S OWN CPU path (oracle/_ref/libvolr_ref.so, built by
`make -C oracle ref` from the sources under /root/reference).  TEST INFRASTRUCTURE.

Run in the build container only (needs /root/reference for Bucky.pvm and oracle/_ref); the fixtures it writes are
data — decoded voxels, parameter blocks, views and rendered frames — and travel with the repo.

What pins what
  * frames / TF / ESL / ray_step / block geometry / decoded Bucky voxels come out of the reference's object code;
  * the Views are produced by this project's host mirror of ViewBase (libvr_hip.so, no GL) and are accepted only if
    the reference frames rendered from them reproduce the FNV-1a32 hashes SURVEY.md §8(c) recorded from the
    reference's own ViewBase.cpp (8 Bucky views at 256x256, default and no-optims) — that pins the camera math.
"""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libvolr_ref.so")
BUCKY = "/root/reference/VolumeRendering/Bucky.pvm"

# hashes captured from the reference incl. its ViewBase.cpp, Bucky @ 256x256
SURVEY_DEFAULT = ["348c8f7b", "0e104dbc", "3cea4ee1", "3ff9f524", "fe1c7adf", "60d78815", "5a251ef4", "96abfe08"]
SURVEY_NOOPT = ["17b84b58", "03a6a6fd", "ec92965a", "6ed01cc9", "fd3753bd", "cbbdbda2", "81a469cc", "525212b1"]
SURVEY_NONZERO = [55296, 51267, 53480, 55520, 34221, 38356, 33409, 33774]
SURVEY_SHELL256 = {"default": ["72d162e6", "1769edd0"], "noopt": ["8bf18ea9", "68d6c9e4"]}


def fnv1a32(buf):
    h = 2166136261
    for b in memoryview(np.ascontiguousarray(buf)).cast("B").tobytes():
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return "%08x" % h


class Ref:
    def __init__(self):
        self.L = C.CDLL(REF_SO)
        self.L.volr_ref_get_voxels.restype = C.POINTER(C.c_ubyte)
        self.L.volr_ref_init()

    def load_model(self, path):
        assert self.L.volr_ref_load_model(path.encode()) == 0
        return self.voxels()

    def voxels(self):
        x, y, z = C.c_uint(), C.c_uint(), C.c_uint()
        self.L.volr_ref_get_dims(C.byref(x), C.byref(y), C.byref(z))
        n = x.value * y.value * z.value
        return np.ctypeslib.as_array(self.L.volr_ref_get_voxels(), shape=(n,)).copy().reshape(z.value, y.value, x.value)

    def set_volume(self, vox):
        vox = np.ascontiguousarray(vox, dtype=np.uint8)
        z, y, x = vox.shape
        assert self.L.volr_ref_set_volume(vox.ctypes.data_as(C.POINTER(C.c_ubyte)), x, y, z) == 0

    def set_base_tf(self, base):
        base = np.ascontiguousarray(base, dtype=np.float32)
        self.L.volr_ref_set_base_transfer_fn(base.ctypes.data_as(C.POINTER(C.c_float)))

    def state(self):
        tf = np.zeros((128, 4), np.float32)
        esl = np.zeros(1024, np.uint32)
        f6 = np.zeros(6, np.float32)
        i2 = np.zeros(2, np.uint32)
        self.L.volr_ref_get_transfer_fn(tf.ctypes.data_as(C.POINTER(C.c_float)))
        self.L.volr_ref_get_esl(esl.ctypes.data_as(C.POINTER(C.c_uint)))
        self.L.volr_ref_get_params(f6.ctypes.data_as(C.POINTER(C.c_float)), i2.ctypes.data_as(C.POINTER(C.c_uint)))
        return tf, esl, f6, i2

    def set_params(self, ray_step, thr, kd, esl):
        self.L.volr_ref_set_params(C.c_float(ray_step), C.c_float(thr), C.c_float(kd), int(esl))

    def render(self, view):
        w, h = view.width, view.height
        v15 = np.array(list(view.origin) + list(view.direction) + list(view.right_plane) + list(view.up_plane) +
                       list(view.light_pos), dtype=np.float32)
        out = np.zeros((h, w, 4), np.uint8)
        rc = self.L.volr_ref_render(w, h, v15.ctypes.data_as(C.POINTER(C.c_float)), int(view.perspective),
                                    out.ctypes.data_as(C.POINTER(C.c_ubyte)), None)
        assert rc == 0
        return out


def view_array(v):
    return np.array([v.width, v.height, v.perspective], np.uint32), np.array(
        list(v.origin) + list(v.direction) + list(v.right_plane) + list(v.up_plane) + list(v.light_pos), np.float32)


def main():
    vr = importlib.import_module("volume-rendering_amd")
    from importlib import import_module
    scene_mod = import_module("volume-rendering_amd.scene")
    os.makedirs(OUT, exist_ok=True)
    ref = Ref()
    arrays, index = {}, {"volumes": {}, "cases": []}

    def add_volume(name, vox, base_tf=None):
        ref.set_volume(vox)
        if base_tf is not None:
            ref.set_base_tf(base_tf)
            arrays[f"vol_{name}_base_tf"] = np.asarray(base_tf, np.float32)
        tf, esl, f6, i2 = ref.state()
        arrays[f"vol_{name}_voxels"] = vox
        arrays[f"vol_{name}_tf"] = tf
        arrays[f"vol_{name}_esl"] = esl
        arrays[f"vol_{name}_f6"] = f6          # ray_step, ray_threshold, light_kd, esl_block_size xyz
        arrays[f"vol_{name}_i2"] = i2          # esl flag, esl_block_dims
        index["volumes"][name] = {"dims_xyz": [int(vox.shape[2]), int(vox.shape[1]), int(vox.shape[0])],
                                  "voxels_fnv1a32": fnv1a32(vox), "esl_popcount": int(sum(bin(int(w)).count("1") for w in esl)),
                                  "custom_tf": base_tf is not None}
        return f6

    def add_case(volume, label, view, ray_step, thr, kd, esl, keep_frame=True):
        ref.set_params(ray_step, thr, kd, esl)
        frame = ref.render(view)
        cid = len(index["cases"])
        dims, v15 = view_array(view)
        arrays[f"case{cid}_viewdims"] = dims
        arrays[f"case{cid}_view"] = v15
        arrays[f"case{cid}_scalars"] = np.array([ray_step, thr, kd], np.float32)
        if keep_frame:
            arrays[f"case{cid}_frame"] = frame
        index["cases"].append({"id": cid, "volume": volume, "label": label, "esl": int(esl), "has_frame": bool(keep_frame),
                               "frame_fnv1a32": fnv1a32(frame), "nonzero_alpha": int((frame[..., 3] != 0).sum())})
        return frame

    # ---------------- Bucky (BASELINE config 1) ----------------
    bucky = ref.load_model(BUCKY)
    assert fnv1a32(bucky) == "70f1ecd5", fnv1a32(bucky)
    bucky.tofile(os.path.join(OUT, "bucky_32.raw"))
    f6 = add_volume("bucky", bucky)
    step = float(f6[0])
    # 256x256: the 8 benchmark views, default + no-optims — must reproduce the survey's hashes (pins ViewBase mirror)
    for i in range(8):
        v = vr.benchmark_view(256, 256, i)
        fr = add_case("bucky", f"bench256_view{i}_default", v, step, 0.95, 0.6, 1)
        assert fnv1a32(fr) == SURVEY_DEFAULT[i], (i, fnv1a32(fr), SURVEY_DEFAULT[i])
        assert int((fr[..., 3] != 0).sum()) == SURVEY_NONZERO[i]
        fr = add_case("bucky", f"bench256_view{i}_nooptims", v, step, 1.0, 0.6, 0)
        assert fnv1a32(fr) == SURVEY_NOOPT[i], (i, fnv1a32(fr), SURVEY_NOOPT[i])
    print("camera mirror pinned: 16/16 Bucky 256x256 frame hashes equal SURVEY §8(c)")
    # 64x64 variants, light off, odd viewport (reference default window 799x715 scaled), camera inside the cube
    for i in range(8):
        add_case("bucky", f"bench64_view{i}_default", vr.benchmark_view(64, 64, i), step, 0.95, 0.6, 1)
    add_case("bucky", "nolight_view1", vr.benchmark_view(96, 96, 1), step, 0.95, 0.0, 1)
    add_case("bucky", "nolight_view5", vr.benchmark_view(96, 96, 5), step, 0.95, 0.0, 1)
    add_case("bucky", "window_199x178_view1", vr.benchmark_view(199, 178, 1), step, 0.95, 0.6, 1)
    add_case("bucky", "window_61x131_view6", vr.benchmark_view(61, 131, 6), step, 0.95, 0.6, 1)
    add_case("bucky", "raystep_x1.7_view3", vr.benchmark_view(128, 128, 3), step * 1.666, 0.95, 0.6, 1)
    add_case("bucky", "raystep_third_view2", vr.benchmark_view(64, 64, 2), step / 3, 0.5, 0.6, 1)
    add_case("bucky", "inside_ortho", scene_mod.custom_view(80, 80, 0, (30, 20, 10), 0.1), step, 0.95, 0.6, 1)
    add_case("bucky", "inside_persp", scene_mod.custom_view(80, 80, 1, (30, 20, 10), 0.1), step, 0.95, 0.6, 1)
    add_case("bucky", "far_persp", scene_mod.custom_view(80, 80, 1, (-120, 200, 33), 3.0), step, 0.95, 0.6, 0)

    # ---------------- synthetic shell, small ----------------
    orc = C.CDLL(os.path.join(ROOT, "oracle", "libvr_oracle.so"))
    shell = np.zeros((48, 48, 48), np.uint8)
    orc.vro_generate_volume(0, 48, 1, 1, shell.ctypes.data_as(C.c_void_p))
    f6 = add_volume("shell48", shell)
    for i in (0, 1, 6, 7):
        add_case("shell48", f"view{i}_default", vr.benchmark_view(96, 96, i), float(f6[0]), 0.95, 0.6, 1)
        add_case("shell48", f"view{i}_nooptims", vr.benchmark_view(96, 96, i), float(f6[0]), 1.0, 0.6, 0)

    # ---------------- non-cubic volume + edited transfer function ----------------
    rng = np.random.RandomState(7)
    zz, yy, xx = np.mgrid[0:56, 0:24, 0:40]
    blob = 255.0 * np.exp(-(((xx - 22) / 13.0) ** 2 + ((yy - 10) / 7.0) ** 2 + ((zz - 30) / 17.0) ** 2))
    vox = np.clip(blob + rng.randint(0, 12, size=blob.shape), 0, 255).astype(np.uint8)
    vox[:8, :, :] = 0                                     # an all-zero slab: ESL-skippable blocks
    base = np.zeros((128, 4), np.float32)
    idx = np.arange(128)
    base[:, 0] = np.abs(np.sin(idx * 0.11))
    base[:, 1] = (idx / 127.0) ** 2
    base[:, 2] = 1.0 - idx / 127.0
    base[:, 3] = np.where((idx > 20) & (idx < 50), 0.02 + idx / 400.0, 0.0) + np.where(idx > 90, 0.7, 0.0)
    f6 = add_volume("blob_40x24x56", vox, base_tf=base.astype(np.float32))
    for i in (1, 2, 5, 7):
        add_case("blob_40x24x56", f"view{i}_default", vr.benchmark_view(120, 72, i), float(f6[0]), 0.95, 0.6, 1)
    add_case("blob_40x24x56", "view3_esl_off", vr.benchmark_view(120, 72, 3), float(f6[0]), 0.9, 1.3, 0)

    # ---------------- BASELINE config 2 hashes only: shell 256^3 @ 1024x1024, ortho poses 0/1 ----------------
    shell256 = np.zeros((256, 256, 256), np.uint8)
    orc.vro_generate_volume(0, 256, 1, 1, shell256.ctypes.data_as(C.c_void_p))
    assert fnv1a32(shell256) == "6d5baf38", fnv1a32(shell256)
    ref.set_volume(shell256)
    tf, esl, f6, i2 = ref.state()
    index["volumes"]["shell256"] = {"dims_xyz": [256, 256, 256], "voxels_fnv1a32": "6d5baf38", "generated": "shell n=256 seed=1",
                                    "esl_popcount": int(sum(bin(int(w)).count("1") for w in esl)), "custom_tf": False}
    arrays["vol_shell256_tf"] = tf
    arrays["vol_shell256_esl"] = esl
    arrays["vol_shell256_f6"] = f6
    arrays["vol_shell256_i2"] = i2
    for i in (0, 1):
        v = vr.benchmark_view(1024, 1024, i)
        fr = add_case("shell256", f"c2_view{i}_default", v, float(f6[0]), 0.95, 0.6, 1, keep_frame=False)
        assert fnv1a32(fr) == SURVEY_SHELL256["default"][i], fnv1a32(fr)
        fr = add_case("shell256", f"c2_view{i}_nooptims", v, float(f6[0]), 1.0, 0.6, 0, keep_frame=False)
        assert fnv1a32(fr) == SURVEY_SHELL256["noopt"][i], fnv1a32(fr)
    print("shell 256^3 @ 1024^2 reference hashes equal SURVEY §8(c)")

    # inputs in golden.npz, frames split by case id parity (tests/helpers.py GOLDEN_SHARDS): every file stays under 1 MiB
    frame_of = lambda k: k.startswith("case") and k.endswith("_frame")
    shards = {"golden.npz": {k: v for k, v in arrays.items() if not frame_of(k)}}
    for p in (0, 1):
        shards[f"golden_frames{p}.npz"] = {k: v for k, v in arrays.items() if frame_of(k) and int(k[4:-6]) % 2 == p}
    for name, part in shards.items():
        np.savez_compressed(os.path.join(OUT, name), **part)
    with open(os.path.join(OUT, "golden.json"), "w") as f:
        json.dump(index, f, indent=1)
    print("wrote", len(index["cases"]), "cases;", {name: os.path.getsize(os.path.join(OUT, name)) // 1024 for name in shards}, "KiB")


if __name__ == "__main__":
    main()
