"""The sampling-point arithmetic of the MSDeformAttn kernels has one definition, trackformer_amd/csrc/msda_point.h: no other
device source retypes the pixel mapping (fma(loc, size, -0.5)) or the module's location formula."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trackformer_amd", "csrc")
# fma(loc, size, -0.5) in any spelling; the first two arguments may hold casts and calls.  (The two-rounding form
# loc * size - 0.5 is not searched for: `* ... - 0.5` is also how the tile geometry maps pixel centres between levels.)
PIXEL_MAPPING = re.compile(r"fma(?:f|_t)?\s*\([^;]*?,\s*(?:\([^()]*\)\s*)?-\s*0\.5")
LOCATION_FORMULA = re.compile(r"ref_dim\s*==\s*2")
ALLOWED = (   # (file, pattern, occurrences, why the site stays)
    ("msda_point.h", PIXEL_MAPPING, 2, "the definition (pixel_point: x and y)"),
    ("msda_point.h", LOCATION_FORMULA, 1, "the definition (fused_location)"),
    ("msda_fused_bwd.h", LOCATION_FORMULA, 1, "the backward epilogue branches on ref_dim for the GRADIENT of the formula (grad / H_l)"),
    # msda_pquad.hip and msda_pquad2.h form off * (1 / H_l) with a reciprocal on purpose (fused_location's comment); they take
    # ref_dim == 2 only and do not branch on it.
    # Sites left with the parent's text because the helper cost registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950;
    # profiles/msda_point_kernel_resources.txt has every kernel):
    ("msda_hip.hip", PIXEL_MAPPING, 2, "direct_body: msda_fwd_f32_direct<2, plain> 71 -> 73 VGPRs, occupancy 7 -> 6"),
    ("msda_fwd_quad.h", PIXEL_MAPPING, 2, "level phase: msda_fwd_f32_quad<fused, 12, 4, 2, 1> scratch 16 -> 28 B, <fused, 12, 4, 3, 15> 12 -> 16 B"),
    ("msda_pquad2.h", PIXEL_MAPPING, 2, "msda_fwd_f32_pquad2<fused, .., cf> scratch 0 -> 32 / 16 B, the other fused ones +4..5 VGPRs"),
)


def test_pixel_mapping_and_location_formula_are_defined_once():
    allowed = {(name, pat): n for name, pat, n, _ in ALLOWED}
    found = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            code = re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
        for pat in (PIXEL_MAPPING, LOCATION_FORMULA):
            n = len(pat.findall(code))
            if n:
                found[(name, pat)] = n
    assert found[("msda_point.h", PIXEL_MAPPING)] == 2 and found[("msda_point.h", LOCATION_FORMULA)] == 1
    extra = {(name, pat.pattern): n for (name, pat), n in found.items() if n > allowed.get((name, pat), 0)}
    assert not extra, extra
