#!/usr/bin/env python3
"""Writes g15_binding_surface.json: the names and signatures of mp3stego._lib at the commit a change of the binding starts from.

Run it on an exported copy of that commit, never on the code under test:

    git archive <parent> | tar -x -C /tmp/parent
    python tests/golden/gen_binding_surface.py /tmp/parent

The file holds the module's non-dunder names, str(inspect.signature()) of every public function, and of every method of Context, Pipe
and StreamIndex.  tests/test_abi.py::test_binding_surface_is_pinned holds today's module against it: a name may be added, a parameter
may be added behind the pinned ones with a default, nothing may go.  Importing the module needs no built library."""
import importlib
import inspect
import json
import os
import sys

CLASSES = ("Context", "Pipe", "StreamIndex")


def methods(cls):
    """{name: signature} of what the class itself defines as functions (static and class methods unwrapped)"""
    out = {}
    for name, v in vars(cls).items():
        v = getattr(v, "__func__", v)
        if inspect.isfunction(v):
            out[name] = str(inspect.signature(v))
    return out


def surface(module):
    names = sorted(n for n in vars(module) if not (n.startswith("__") and n.endswith("__")))
    functions = {n: str(inspect.signature(getattr(module, n))) for n in names
                 if not n.startswith("_") and inspect.isfunction(getattr(module, n))}
    return {"names": names, "functions": functions, "methods": {c: methods(getattr(module, c)) for c in CLASSES}}


if __name__ == "__main__":
    root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, os.path.join(root, "mp3-steganography-lib_amd"))
    module = importlib.import_module("mp3stego._lib")
    assert os.path.abspath(module.__file__).startswith(root), module.__file__
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g15_binding_surface.json")
    with open(out, "w") as f:
        json.dump(surface(module), f, indent=1, sort_keys=True)
        f.write("\n")
    s = surface(module)
    print(out, len(s["names"]), "names,", len(s["functions"]), "functions,", sum(len(m) for m in s["methods"].values()), "methods")
