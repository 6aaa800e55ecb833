"""Writes tests/golden/so100_cameras.json and tests/golden/aloha_cameras.json: the <camera> elements of the reference's scenes as plain settings.

    python scripts/make_golden_cameras.py /path/to/so101_sim/assets/so100/scene_pbr.xml
    python scripts/make_golden_cameras.py --aloha /path/to/so101_sim/assets/aloha/scene_pbr.xml /path/to/so101_sim/assets/aloha/aloha_pbr.xml

Per camera: name, the body it is fixed to, that body's chain of (name, pos, quat) up to the world, and the camera's own
pos / xyaxes / fovy attributes exactly as the MJCF states them (null where the attribute is absent and MuJoCo's default
applies: identity orientation, fovy 45).  tests/test_render_emu.py composes these and compares them with
so101_sim_amd.cameras.SO100_CAMERAS.

--aloha: the scene file and the robot file it includes, in that order; the records also carry the camera's quat / euler / focal /
sensorsize attributes, a body's record its euler, and the file states the robot file's <compiler angle>.  tests/test_tree_render_emu.py
compares them with so101_sim_amd.cameras.ALOHA_CAMERAS.
"""
import json
import os
import sys
import xml.etree.ElementTree as ET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def floats(text):
    return None if text is None else [float(x) for x in text.split()]


def cameras_of(path, camera_attrs=("pos", "xyaxes", "fovy"), body_attrs=("pos", "quat")):
    root = ET.parse(path).getroot()
    cams = []

    def walk(elem, chain):
        for c in elem.findall("camera"):
            cams.append(dict(name=c.get("name"), body=chain[-1]["name"] if chain else "world", chain=list(chain),
                             **{a: floats(c.get(a)) for a in camera_attrs}))
        for b in elem.findall("body"):
            walk(b, chain + [dict(name=b.get("name"), **{a: floats(b.get(a)) for a in body_attrs})])

    walk(root.find("worldbody"), [])
    return root, cams


def write(name, out):
    dst = os.path.join(ROOT, "tests", "golden", name)
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(dst, len(out["cameras"]), "cameras")


def main(path):
    _, cams = cameras_of(path)
    write("so100_cameras.json", dict(source="so101_sim/assets/so100/scene_pbr.xml", default_fovy=45.0, cameras=cams))


def main_aloha(scene, robot):
    attrs = ("pos", "xyaxes", "fovy", "quat", "euler", "focal", "sensorsize")
    cams, angle = [], None
    for path, source in ((scene, "so101_sim/assets/aloha/scene_pbr.xml"), (robot, "so101_sim/assets/aloha/aloha_pbr.xml")):
        root, found = cameras_of(path, attrs, ("pos", "quat", "euler"))
        comp = root.find("compiler")
        if comp is not None and comp.get("angle"):
            angle = comp.get("angle")
        cams += [dict(c, source=source) for c in found]
    write("aloha_cameras.json", dict(source=["so101_sim/assets/aloha/scene_pbr.xml", "so101_sim/assets/aloha/aloha_pbr.xml"], default_fovy=45.0,
                                     angle=angle, cameras=cams))


if __name__ == "__main__":
    if sys.argv[1] == "--aloha":
        main_aloha(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1])
