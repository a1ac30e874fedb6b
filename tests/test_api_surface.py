"""The Python surface is pinned: the signature of every public function of
api.py and of every public method of its classes, and the public names of the
package, against the committed listing tests/api_surface.json (no GPU, no
librm.so).  A change to the listing is a change of the public interface and is
made on purpose: `PYTHONPATH=. python tests/test_api_surface.py` rewrites it
from the code."""
import inspect
import json
import os

import raymarching_amd as rm
from raymarching_amd import api

LISTING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "api_surface.json")
CLASSES = ("Renderer", "Comm", "Shader", "ShaderLoader", "RenderTexture")


def surface() -> dict:
    functions = {n: str(inspect.signature(f)) for n, f in vars(api).items()
                 if inspect.isfunction(f) and f.__module__ == api.__name__ and not n.startswith("_")}
    classes = {}
    for c in CLASSES:
        cls = getattr(api, c)
        members = {"__init__": str(inspect.signature(cls))}
        for n, raw in vars(cls).items():  # the class's own members; Shader's inherited ones are Renderer's
            if n.startswith("_"):
                continue
            if isinstance(raw, property):
                members[n] = "property"
            elif callable(getattr(cls, n)):
                kind = {staticmethod: "static ", classmethod: "class "}.get(type(raw), "")
                members[n] = kind + str(inspect.signature(getattr(cls, n)))
        classes[c] = members
    names = sorted(n for n in dir(rm) if not n.startswith("_") and not inspect.ismodule(getattr(rm, n)))
    return {"functions": functions, "classes": classes, "package_names": names}


def test_api_signatures_are_the_listed_ones():
    want, got = json.load(open(LISTING)), surface()
    assert got["functions"] == want["functions"]
    assert got["classes"] == want["classes"]


def test_package_names_are_the_listed_ones():
    assert surface()["package_names"] == json.load(open(LISTING))["package_names"]


if __name__ == "__main__":
    with open(LISTING, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
