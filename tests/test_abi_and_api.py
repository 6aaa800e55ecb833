"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports everything
include/so101.h declares, rejects bad blobs without touching a GPU, and the Python registry/factory
behaves like so101_sim/task_suite.py."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(hip_lib):
    from so101_sim_amd import native
    header = open(os.path.join(ROOT, "include", "so101.h")).read()
    declared = set(re.findall(r"\b(so101_[a-z_]+)\s*\(", header))
    assert declared == set(native.EXPORTS)
    lib = native.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.so101_version() == 10 and lib.so101_max_contacts() >= 16


def _header_prototypes():
    """[(return type, name, [parameter, ...])] of every so101_* prototype of include/so101.h, comments and preprocessor lines removed first
    (prototypes carry comments with commas inside their parameter lists)"""
    text = open(os.path.join(ROOT, "include", "so101.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*$", " ", text, flags=re.M)
    out = []
    for ret, name, params in re.findall(r"(?:^|[;{}])\s*([A-Za-z_][\w\s\*]*?)\s*\b(so101_\w+)\s*\(([^()]*)\)\s*(?=;)", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        out.append((" ".join(ret.split()), name, [] if params == ["void"] else params))
    return out


def _ctype_class(t):
    """(kind, bytes) of a ctypes type: compared by kind and size, not identity (c_size_t is c_uint64 here)"""
    import ctypes as C
    if t is None:
        return ("void", 0)
    if issubclass(t, C._Pointer) or t in (C.c_void_p, C.c_char_p):
        return ("pointer", C.sizeof(t))
    code = t._type_
    kind = "float" if code in "fd" else "signed" if code in "bhilq" else "unsigned" if code in "BHILQ" else code
    return (kind, C.sizeof(t))


C_CLASSES = {"int": ("signed", 4), "int32_t": ("signed", 4), "size_t": ("unsigned", 8), "uint64_t": ("unsigned", 8), "float": ("float", 4)}
C_RETURNS = {"int": "c_int", "void": None, "const char*": "c_char_p", "long long": "c_longlong"}


def test_signature_table_matches_the_header():
    """native.SIGNATURES against the prototypes of include/so101.h: the same 63 names, and per parameter and return value the same class
    (pointer, 4-byte signed, 8-byte unsigned, float); a POINTER(Structure) only where the header names the struct that Structure mirrors,
    and a struct pointer of the header never as a bare address."""
    import ctypes as C
    from so101_sim_amd import native
    protos = _header_prototypes()
    assert len(protos) == 63 and len({p[1] for p in protos}) == 63
    assert {p[1] for p in protos} == set(native.SIGNATURES)
    mirrored = {c: s for s, names in native.C_STRUCTS.items() for c in names}
    for ret, name, params in protos:
        restype, argtypes = native.SIGNATURES[name]
        want = C_RETURNS[ret.replace(" *", "*")]
        assert restype is (getattr(C, want) if want else None), (name, ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for k, (p, t) in enumerate(zip(params, argtypes)):
            where = (name, k, p, t)
            if "*" in p:
                assert _ctype_class(t)[0] == "pointer", where
                ctype = p.replace("const ", "").split("*")[0].strip()
                if issubclass(t, C._Pointer) and issubclass(t._type_, C.Structure):
                    assert ctype in native.C_STRUCTS[t._type_], where
                elif ctype in mirrored:
                    assert False, ("a struct pointer typed as a bare address", where)
            else:
                assert _ctype_class(t) == C_CLASSES[p.replace("const ", "").rsplit(" ", 1)[0]], where


def _layout_fields(struct, prefix="", base=0):
    """[(member path, offset, size)] of a ctypes Structure; arrays of structures are walked element by element"""
    import ctypes as C
    out = []
    for fname, ftype in struct._fields_:
        f = getattr(struct, fname)
        if issubclass(ftype, C.Array) and issubclass(ftype._type_, C.Structure):
            for k in range(ftype._length_):
                out += _layout_fields(ftype._type_, f"{prefix}{fname}[{k}].", base + f.offset + k * C.sizeof(ftype._type_))
        else:
            out.append((prefix + fname, base + f.offset, f.size))
    return out


def test_struct_layouts_match_the_header():
    """sizeof and every field's offset and size of the ctypes Structures against the structs of include/so101.h, as the host compiler lays them
    out: a generated program prints them (LightSpec through the member paths of so101_shading.light[k])."""
    import ctypes as C
    import subprocess
    from so101_sim_amd import native
    from tests import devprims
    assert set(native.C_STRUCTS) == {native.Buffers, native.Config, native.CameraSpec, native.ShadingSpec, native.ColorOut, native.ToolSpec, native.IkConfig,
                                     native.TreeIkConfig, native.GeomPair, native.TreeGeomPair, native.ContactOut, native.ProximityOut, native.TreeConfig}
    want, lines = {}, []
    for struct, cnames in native.C_STRUCTS.items():
        for c in cnames:
            want[c] = (C.sizeof(struct), 0)
            lines.append(f'  std::printf("{c} %zu 0\\n", sizeof({c}));')
            for path, offset, size in _layout_fields(struct):
                want[f"{c}.{path}"] = (offset, size)
                lines.append(f'  std::printf("{c}.{path} %zu %zu\\n", offsetof({c}, {path}), sizeof((({c}*)0)->{path}));')
    assert want["so101_shading.light[3].headlight"][1] == 4 and C.sizeof(native.LightSpec) * native.MAX_LIGHTS == native.ShadingSpec.light.size
    text = '#include <cstddef>\n#include <cstdio>\n#include "so101.h"\nint main() {\n' + "\n".join(lines) + "\n  return 0;\n}\n"
    os.makedirs(devprims.OUT, exist_ok=True)
    src = os.path.join(devprims.OUT, "abi_layout.cpp")
    tmp = f"{src}.{os.getpid()}.tmp"
    with open(tmp, "w") as f:
        f.write(text)
    os.replace(tmp, src)
    exe = devprims.cached_build(src, "host", extra_inputs=[os.path.join(ROOT, "include", "so101.h")], program=True)
    got = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        name, a, b = line.split()
        got[name] = (int(a), int(b))
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


SURFACE_CLASSES = {"env": ("BatchedEnvironment", "SingleEnvironment", "SO100HandOverTask"),
                   "aloha": ("AlohaEnvironment", "HandOverTask", "DiningPlaceInContainerTask"), "native": ("Sim", "TreeSim")}


def python_surface() -> dict:
    """{module.Class: {public callable or __init__: [str(inspect.signature), sha256 of inspect.getdoc]}} of the classes a caller sees
    (scripts/make_golden_python_surface.py writes it to tests/golden/python_surface.json)"""
    import hashlib
    import importlib
    import inspect
    out = {}
    for mod, classes in SURFACE_CLASSES.items():
        m = importlib.import_module("so101_sim_amd." + mod)
        for cname in classes:
            cls = getattr(m, cname)
            names = ["__init__"] + [n for n in dir(cls) if not n.startswith("_") and callable(getattr(cls, n))]
            out[f"{mod}.{cname}"] = {n: [str(inspect.signature(getattr(cls, n))), hashlib.sha256((inspect.getdoc(getattr(cls, n)) or "").encode()).hexdigest()]
                                     for n in names}
    return out


def test_python_surface_is_the_pinned_one():
    """Names, signatures and docstrings of the public methods of the environment, task and handle classes are those of
    tests/golden/python_surface.json (dumped from the commit before the host layer was unified)."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "python_surface.json")))
    got = python_surface()
    assert set(got) == set(want)
    # the one addition since the dump: synchronize() moved to the base of both environment classes, so AlohaEnvironment has it as well
    assert got["aloha.AlohaEnvironment"].pop("synchronize") == want["env.BatchedEnvironment"]["synchronize"]
    for cls in want:
        assert got[cls] == want[cls], (cls, {n for n in set(got[cls]) | set(want[cls]) if got[cls].get(n) != want[cls].get(n)})


def test_create_rejects_bad_blobs_without_gpu(hip_lib, blobs):
    from so101_sim_amd import native
    with pytest.raises(RuntimeError, match="bad blob magic"):
        native.Sim(b"\0" * 64, 4)
    with pytest.raises(RuntimeError, match="f32 blob"):
        native.Sim(blobs["f64"], 4)
    with pytest.raises(RuntimeError, match="truncated"):
        native.Sim(blobs["f32"][:4000], 4)
    lib = native.load_library()
    assert lib.so101_configure(None, None) == -1 and lib.so101_step(None, None, None, None, None, None, None) == -1
    # a mesh geom without vertices (the support tables and queries need one): rejected by the model check, which runs after the device
    # is made current - so through the emulated build of the same source (tests/hostemu), which needs no GPU
    from tests.simharness import build_emu
    emu = build_emu()
    for n in (0, -1):
        with pytest.raises(RuntimeError, match=r"so101_create failed \(-2\): mesh geom without vertices"):
            native.Sim(_with_mesh_vertnum(blobs["f32"], n), 4, lib_path=emu)


def _with_mesh_vertnum(raw, n):
    """the blob with geom_vertnum of its first mesh geom set to n"""
    from so101_sim_amd.model import blob as blobfmt
    m = blobfmt.unpack(raw)
    vn = m["geom_vertnum"].copy()
    vn[int(np.flatnonzero(m["geom_type"] == 5)[0])] = n
    m["geom_vertnum"] = vn
    return blobfmt.pack(m)


def test_tree_create_rejects_mesh_without_vertices_without_gpu():
    from so101_sim_amd import native
    from so101_sim_amd.model import scenes
    from tests.simharness import build_emu
    emu = build_emu()
    raw = scenes.load_aloha_blob("banana", "f32")[0]
    for n in (0, -1):
        with pytest.raises(RuntimeError, match=r"so101_tree_create failed \(-2\): mesh geom without vertices"):
            native.TreeSim(_with_mesh_vertnum(raw, n), 4, lib_path=emu)


def test_missing_library_fails_loudly(tmp_path):
    from so101_sim_amd import native
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.load_library(str(tmp_path / "nope.so"))


def test_product_never_imports_the_oracle():
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "so101_sim_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                text = open(os.path.join(base, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", text, re.M) or "so101_oracle" in text or "oracle/" in text:
                    bad.append(f)
    assert not bad, bad


def test_registry_matches_reference_names():
    from so101_sim_amd import task_suite
    keys = list(task_suite.TASK_FACTORIES.keys())
    assert len(keys) == 22
    assert keys[:3] == ["BlocksSpelling", "BowlOnRack", "DesktopWrapHeadphone"] and keys[-2:] == ["SO100HandOverPen", "SO100HandOverBanana"]
    assert task_suite.TASK_FACTORIES["SO100HandOverBanana"][1] == {"object_name": "banana"}
    assert task_suite.DEFAULT_CONTROL_TIMESTEP == 0.02
    assert task_suite.DEFAULT_CAMERAS == ("overhead_cam", "worms_eye_cam", "wrist_cam_left", "wrist_cam_right")


def test_reference_import_path_works_without_an_install_call():
    """`from so101_sim import task_suite` (run_eval.py:22, scripts/so101_lerobot_wrapper.py:12, so101_rl.ipynb) resolves to this build from a fresh
    interpreter with the repo root on the path - no install_as_so101_sim() line - and hands out the SAME registry and factory objects."""
    import subprocess
    import sys
    code = ("from so101_sim import task_suite\n"
            "import so101_sim, so101_sim_amd.task_suite as t\n"
            "assert task_suite.create_task_env is t.create_task_env and task_suite.TASK_FACTORIES is t.TASK_FACTORIES\n"
            "assert so101_sim.task_suite is task_suite and len(task_suite.TASK_FACTORIES) == 22\n"
            "assert task_suite.DEFAULT_CONTROL_TIMESTEP == 0.02 and task_suite.SO100HandOver is t.SO100HandOver\n"
            "try:\n    task_suite.create_task_env('Nope', time_limit=1.0)\nexcept ValueError as e:\n    assert 'Unknown task_name: Nope' in str(e)\nelse:\n    raise SystemExit(3)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr
    # nothing of the reference lives in the alias package: two short files that import so101_sim_amd
    files = sorted(f for f in os.listdir(os.path.join(ROOT, "so101_sim")) if not f.startswith("__pycache__"))
    assert files == ["__init__.py", "task_suite.py"]
    assert all(len(open(os.path.join(ROOT, "so101_sim", f)).read().splitlines()) < 20 for f in files)


def test_factory_errors_like_reference():
    from so101_sim_amd import task_suite
    with pytest.raises(ValueError, match="Unknown task_name: Nope. Available tasks:"):
        task_suite.create_task_env("Nope", time_limit=1.0)
    with pytest.raises(NotImplementedError):
        task_suite.create_task_env("BowlOnRack", time_limit=1.0)              # ALOHA tasks other than the hand-over: registry key exists, not built
    assert task_suite.HandOver(object_name="banana", reward_based_on_overlap=False, reward_requires_handover=True).reward_requires_handover
    with pytest.raises(ValueError, match="Invalid object name"):
        task_suite.HandOver(object_name="mug")
    t = task_suite.HandOver(object_name="pen", control_timestep=0.02, cameras=())
    assert t.get_instruction() == "hand over the pen and put it in the container"       # hand_over.py:117
    with pytest.raises(ValueError, match="Invalid object name"):
        task_suite.SO100HandOver(object_name="mug")


def test_task_kwargs_and_calibration_cwd_quirk(tmp_path, monkeypatch):
    from so101_sim_amd import task_suite
    monkeypatch.chdir(tmp_path)
    t = task_suite.SO100HandOver(object_name="banana", control_timestep=0.02, cameras=())
    assert np.all(t.calibration.homing_offsets == 0)                            # file not found -> zeros, silently
    assert t.get_instruction() == "pick up the banana and put it in the bowl using the SO100 arm"
    os.makedirs(tmp_path / "calibration")
    (tmp_path / "calibration" / "red_arm.json").write_text(
        '{"shoulder_pan": {"homing_offset": 28}, "shoulder_lift": {"homing_offset": 42}, "elbow_flex": {"homing_offset": 18},'
        ' "wrist_flex": {"homing_offset": -21}, "wrist_roll": {"homing_offset": 1009}, "gripper": {"homing_offset": -158}}')
    t = task_suite.SO100HandOver(object_name="banana")
    assert list(t.calibration.homing_offsets) == [28, 42, 18, -21, 1009, -158]
    with pytest.raises(ValueError, match="Expected 6 joint positions, got 5"):
        t.calibration.apply_calibration_to_action(np.zeros(5))


def test_dmenv_lookalikes():
    from so101_sim_amd._dmenv import StepType, TimeStep
    ts = TimeStep(StepType.FIRST, None, None, {})
    assert ts.first() and not ts.mid() and not ts.last() and ts.reward is None and ts.discount is None
    assert TimeStep(StepType.LAST, 1.0, 0.0, {}).last()


def test_shard_ranges_partition_the_envs():
    from so101_sim_amd.distributed import shard_range
    for n, w in ((262144, 8), (4096, 2), (10, 3)):
        spans = [shard_range(n, w, r) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


def test_lerobot_packaging_format():
    """so101_lerobot_wrapper.py:77-122: keys, dtypes, the 0.1 s timestamp quirk, zero action on reset; batched shapes."""
    import numpy as np
    import torch
    from so101_sim_amd import lerobot
    o = lerobot.to_lerobot_format(np.arange(6, dtype=np.float64), None, 0, 3)
    assert set(o) == {"observation.state", "action", "timestamp", "frame_index", "episode_index", "index", "task_index", "task"}
    assert o["observation.state"].dtype == torch.float32 and o["observation.state"].shape == (6,)
    assert torch.equal(o["action"], torch.zeros(6)) and o["timestamp"].item() == 0.0 and o["episode_index"].item() == 3
    o = lerobot.to_lerobot_format(np.zeros(6), np.ones(6), 7, 0)
    assert abs(o["timestamp"].item() - 0.7) < 1e-6 and o["frame_index"].item() == 7 and o["index"].item() == 7
    assert o["frame_index"].dtype == torch.long and o["task"] == "SO100 manipulation task" and o["task_index"].item() == 0
    b = lerobot.to_lerobot_format(np.zeros((5, 6)), None, 2, 1, n_envs=5)
    assert b["observation.state"].shape == (5, 6) and b["action"].shape == (5, 6) and b["frame_index"].shape == (5,)
    assert torch.all(b["frame_index"] == 2) and torch.allclose(b["timestamp"], torch.full((5,), 0.2))


def test_lerobot_packaging_matches_the_reference_wrapper():
    """tests/golden/lerobot_cases.json holds outputs of the reference's own SO101LeRobotWrapper._convert_to_lerobot_format
    (scripts/make_golden_lerobot.py executes it on synthetic time steps): same keys, dtypes, shapes and bit-identical
    values from so101_sim_amd.lerobot.to_lerobot_format."""
    import json
    import numpy as np
    import torch
    from so101_sim_amd.lerobot import to_lerobot_format
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "lerobot_cases.json")))
    assert len(g["cases"]) >= 10
    for c in g["cases"]:
        act = None if c["action"] is None else np.asarray(c["action"], dtype=c["action_dtype"])
        out = to_lerobot_format(np.asarray(c["joints_pos"]), act, c["frame_index"], c["episode_index"], device="cpu", n_envs=1)
        assert set(out) == set(c["expected"]), (set(out) ^ set(c["expected"]))
        for k, want in c["expected"].items():
            if isinstance(want, str):
                assert out[k] == want
                continue
            got = out[k]
            assert str(got.dtype) == want["dtype"] and list(got.shape) == want["shape"], (k, got.dtype, got.shape, want)
            assert got.double().flatten().tolist() == want["value"], k


def test_settled_cache_file_format(tmp_path):
    """Host logic of the on-disk settled-state store: round trip, key check, damage detection."""
    from so101_sim_amd import settled_cache as sc
    E, N = 3, 5
    rng = np.random.RandomState(0)
    arrays = {"qpos": rng.randn(E, 20, N).astype(np.float32), "qvel": rng.randn(E, 18, N).astype(np.float32),
              "warmstart": rng.randn(E, 18, N).astype(np.float32), "flags": rng.randint(0, 64, size=(E, N)).astype(np.int32)}
    key = {"seed": 7, "blob_sha256": "ab", "env_id_base": 4096, "action_offset": [0.0] * 6, "build": "x"}
    path = str(tmp_path / "s.bin")
    sc.write(path, key, 2, arrays)
    header, got = sc.read(path, expect_key=dict(key))
    assert header["first_episode"] == 2 and header["n_episodes"] == E and header["n_envs"] == N
    for k in arrays:
        np.testing.assert_array_equal(got[k], arrays[k])
        assert got[k].dtype == arrays[k].dtype
    with pytest.raises(sc.SettledCacheError, match="env_id_base"):          # another shard's file
        sc.read(path, expect_key=dict(key, env_id_base=0))
    with pytest.raises(sc.SettledCacheError, match="build"):
        sc.read(path, expect_key=dict(key, build="y"))
    data = bytearray(open(path, "rb").read())
    data[len(data) // 2] ^= 1
    open(path, "wb").write(bytes(data))
    with pytest.raises(sc.SettledCacheError, match="checksum"):
        sc.read(path)
    open(path, "wb").write(bytes(data[:100]))
    with pytest.raises(sc.SettledCacheError):
        sc.read(path)
    with pytest.raises(sc.SettledCacheError, match="shape"):
        sc.write(path, key, 0, dict(arrays, qpos=arrays["qpos"][:, :19]))


def test_aloha_action_spec():
    """AlohaTask.action_spec (aloha2_task.py:279-301) from the compiled model's ctrlrange."""
    from so101_sim_amd import aloha
    from so101_sim_amd.model import blob as blobfmt, scenes
    m = blobfmt.unpack(scenes.load_aloha_blob("banana", "f32")[0])
    spec = aloha.aloha_action_spec(np.asarray(m["act_ctrlrange"], dtype=np.float64).reshape(-1, 2))
    assert spec.shape == (14,) and spec.dtype == np.float32
    assert spec.minimum[0] == spec.minimum[7] == np.float32(-np.pi / 2) and spec.maximum[0] == np.float32(np.pi / 2)
    assert spec.minimum[6] == spec.minimum[13] == np.float32(-0.06135) and spec.maximum[6] == spec.maximum[13] == np.float32(1.5155)
    np.testing.assert_allclose(spec.minimum[1:6], [-1.85005, -1.76278, -3.14158, -1.8675, -3.14158], rtol=1e-6)
    np.testing.assert_allclose(spec.maximum[8:13], [1.25664, 1.6057, 3.14158, 2.23402, 3.14158], rtol=1e-6)
