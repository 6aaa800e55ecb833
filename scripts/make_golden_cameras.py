"""Writes tests/golden/so100_cameras.json: the <camera> elements of the reference's SO100 scene as plain settings.

    python scripts/make_golden_cameras.py /path/to/so101_sim/assets/so100/scene_pbr.xml

Per camera: name, the body it is fixed to, that body's chain of (name, pos, quat) up to the world, and the camera's own
pos / xyaxes / fovy attributes exactly as the MJCF states them (null where the attribute is absent and MuJoCo's default
applies: identity orientation, fovy 45).  tests/test_render_emu.py composes these and compares them with
so101_sim_amd.cameras.SO100_CAMERAS.
"""
import json
import os
import sys
import xml.etree.ElementTree as ET


def floats(text):
    return None if text is None else [float(x) for x in text.split()]


def main(path):
    root = ET.parse(path).getroot()
    cams = []

    def walk(elem, chain):
        for c in elem.findall("camera"):
            cams.append(dict(name=c.get("name"), body=chain[-1]["name"] if chain else "world", chain=list(chain),
                             pos=floats(c.get("pos")), xyaxes=floats(c.get("xyaxes")), fovy=floats(c.get("fovy"))))
        for b in elem.findall("body"):
            walk(b, chain + [dict(name=b.get("name"), pos=floats(b.get("pos")), quat=floats(b.get("quat")))])

    walk(root.find("worldbody"), [])
    out = dict(source="so101_sim/assets/so100/scene_pbr.xml", default_fovy=45.0, cameras=cams)
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "so100_cameras.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(dst, len(cams), "cameras")


if __name__ == "__main__":
    main(sys.argv[1])
