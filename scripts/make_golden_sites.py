"""Writes tests/golden/aloha_sites.json: the named <site> elements of the reference's ALOHA robot file as plain settings.

    python scripts/make_golden_sites.py /path/to/so101_sim/assets/aloha/aloha_pbr.xml

Per site: name, the body it is fixed to, and its pos / quat attributes exactly as the MJCF states them (null where the attribute is
absent and MuJoCo's default applies: the body's origin, the body's own axes).  tests/test_tree_tool_emu.py compares them with
so101_sim_amd.tools.ALOHA_TOOLS.  Runs where the reference's assets are; the fixture holds data only.
"""
import json
import os
import sys
import xml.etree.ElementTree as ET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def floats(text):
    return None if text is None else [float(x) for x in text.split()]


def sites_of(path):
    sites = []

    def walk(elem, body):
        for s in elem.findall("site"):
            if s.get("name"):
                sites.append(dict(name=s.get("name"), body=body, pos=floats(s.get("pos")), quat=floats(s.get("quat"))))
        for b in elem.findall("body"):
            walk(b, b.get("name"))

    walk(ET.parse(path).getroot().find("worldbody"), "world")
    return sites


def main(path):
    out = dict(source="so101_sim/assets/aloha/aloha_pbr.xml", sites=sites_of(path))
    dst = os.path.join(ROOT, "tests", "golden", "aloha_sites.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(dst, len(out["sites"]), "sites")


if __name__ == "__main__":
    main(sys.argv[1])
