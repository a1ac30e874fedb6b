#!/usr/bin/env python3
"""Fixtures of the generalised post.frag pass (rm_post_frag):
the reference's post.frag rendered by SwiftShader with the one statement of its
main() replaced by a choice of sample and tonemap operator.

The shader text is built at run time from the reference checkout (--ref) and is
not stored: POSTFRAG_<input>.npz holds `input`, one `<sample>_<tonemap>` output
per combination and `meta`.  The texture coordinate is the exact pixel-centre
value (EXACT_TC of make_goldens.py), which is what the restatement
(tests/post_frag_ref.py) and the HIP pass compute.

Usage: python tests/golden/make_post_goldens.py --ref DIR [--only NAME]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_goldens import EXACT_TC, GL, fxaa_inputs, must_sub, post_fxaa, unorm8  # noqa: E402,F401
from post_frag_ref import POST_SAMPLES, TONEMAPS  # noqa: E402

SAMPLE_GLSL = {
    "fxaa": "color = fxaa(u_main_tex, uv, u_resolution);",
    "texel": "color = texture(u_main_tex, uv);",
    "chromatic": "color = vec4(chromaticAberration(u_main_tex, uv), texture(u_main_tex, uv).a);",
}
TONEMAP_GLSL = {"none": None, "aces": "tonemapACES", "reinhard": "tonemapReinhard", "jodie": "tonemapReinhardJodie",
                "uncharted2": "tonemapUncharted2Filmic"}


def post_frag_glsl(ref: str, sample: str, tonemap: str) -> str:
    s = post_fxaa(ref)
    s = must_sub("vec4(v_uv, 0.0, 0.0)", f"vec4({EXACT_TC}, 0.0, 0.0)", s)
    line = SAMPLE_GLSL[sample]
    if TONEMAP_GLSL[tonemap]:
        line += f"\n\tcolor.rgb = {TONEMAP_GLSL[tonemap]}(color.rgb);"
    stmt = "color = fxaa(u_main_tex, uv, u_resolution);"
    return s if line == stmt else must_sub(stmt, line, s)


def noise_inputs():
    """Full 32-bit random words (alpha random too), one even and one odd size."""
    rng = np.random.default_rng(20261019)
    out = []
    for W, H in ((96, 64), (61, 37)):
        out.append((f"noise_{W}x{H}", rng.integers(0, 2**32, (H, W), dtype=np.uint64).astype(np.uint32)))
    return out


def inputs():
    """(name, image, with_fxaa): noise is no fixture for the FXAA branch (the
    FXAA restatement's own policy does not hold on noise)."""
    return [(n, img, True) for n, img in fxaa_inputs()] + [(n, img, False) for n, img in noise_inputs()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference (cahekp/Raymarching)")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    for name, img, with_fxaa in inputs():
        if args.only and args.only not in name:
            continue
        H, W = img.shape
        g = GL(W, H)
        arrs = {}
        for sample in POST_SAMPLES:
            if sample == "fxaa" and not with_fxaa:
                continue
            for tm in TONEMAPS:
                arrs[f"{sample}_{tm}"] = g.post(g.program(post_frag_glsl(args.ref, sample, tm)), img, (W, H))
        meta = dict(pass_="post.frag main() with sample x tonemap", W=W, H=H, sampler="NEAREST, CLAMP_TO_EDGE",
                    texcoord="exact pixel centre", combos=sorted(arrs), renderer=g.renderer,
                    generator="tests/golden/make_post_goldens.py")
        path = os.path.join(HERE, f"POSTFRAG_{name}.npz")
        np.savez_compressed(path, input=img, meta=json.dumps(meta), **arrs)
        print(f"POSTFRAG_{name}: {len(arrs)} outputs, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
