"""Writes tests/golden/python_surface.json: per public class {public callable: signature, sha256 of its docstring}, as
tests/test_abi_and_api.py::python_surface computes it.  Run it from a checkout of the commit whose surface is to be pinned (the parent of a
refactor), with the repository root as the working directory; needs no GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_abi_and_api import python_surface          # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "python_surface.json")
    with open(out, "w") as f:
        json.dump(python_surface(), f, indent=1, sort_keys=True)
        f.write("\n")
