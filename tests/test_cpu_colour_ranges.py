"""The value ranges the fused encoder's colour arithmetic rests on (encode.hip
ycc8, round 11): the Cb word never leaves 24 bits, so it carries no clamp; the Cr
word does at exactly three inputs, so it keeps its own.  Exhaustive over all 2^24
RGB triples (tools/check/colour_dot4.py ranges())."""
import importlib.util
import os


def test_fused_colour_cb_needs_no_clamp():
    spec = importlib.util.spec_from_file_location(
        "colour_dot4", os.path.join(os.path.dirname(__file__), "..", "tools", "check", "colour_dot4.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.ranges()
