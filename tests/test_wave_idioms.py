"""csrc/wave.hpp is the one place for the wave-level idioms: plain text over visfd_amd/csrc, so the copies do not grow back."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "visfd_amd", "csrc")

# the units that take their wave size, lane and helpers from the header
CONVERTED = ["intensity.hip", "discard_overlap.hip", "connect_graph.hip", "surface_points.hip", "find_spheres.hip", "distance.hip",
             "close_surface.hip", "voxelize.hip", "draw.hip", "extrema.hip", "watershed.hip", "morph_levels.hip", "median.hip",
             "ridge.hip", "blob.hip"]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _defined(text):
    """names of the device functions a file defines"""
    return set(re.findall(r"^[^\n/]*__device__[^\n(]*?\b(\w+)\s*\(", text, re.M))


def test_header_names_are_defined_once():
    names = _defined(_read("wave.hpp"))
    assert {"wave_lane", "wave_reduce", "wave_sum", "wave_min", "wave_max", "wave_or", "wave_scan", "wave_leader", "wave_rank",
            "wave_append", "wave_agree"} <= names
    for f in sorted(os.listdir(CSRC)):
        if f == "wave.hpp":
            continue
        again = names & _defined(_read(f))
        assert not again, "%s defines %s, which csrc/wave.hpp has" % (f, sorted(again))


def test_no_unit_defines_a_wave_helper_of_its_own():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            own = sorted(n for n in _defined(_read(f)) if n.startswith("wave_"))
            assert not own, "%s defines %s: it belongs in csrc/wave.hpp" % (f, own)


def test_converted_units_take_the_wave_size_from_the_header():
    for f in CONVERTED:
        text = _read(f)
        assert '#include "wave.hpp"' in text, f
        own = re.findall(r"\w*WAVE\w*\s*=\s*64", text)
        assert not own, "%s defines %s" % (f, own)
