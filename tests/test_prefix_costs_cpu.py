"""CPU: the entry points of SEMANTICS.md §3k as include/eppk.h declares them against the ctypes prototypes of _lib.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["eppk_prefix_costs_device", "eppk_prefix_costs", "eppk_pick_cost_cached_device", "eppk_pick_cost_cached"]


def test_header_and_binding_agree_on_the_new_prototypes():
    with open(os.path.join(ROOT, "include", "eppk.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    with open(os.path.join(ROOT, "gateway-api-inference-extension_amd", "_lib.py")) as f:
        src = f.read()
    ctype = {"uint32_t": "u32"}                                             # every other parameter of these calls is a pointer
    for name in NEW:
        params = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1).split(",")
        want = ["vp" if "*" in p else ctype[p.split()[0]] for p in params]
        if "const eppk_band_table*" in " ".join(params):
            want[[i for i, p in enumerate(params) if "eppk_band_table" in p][0]] = "C.POINTER(BandTable)"
        got = re.search(r"lib\.%s\.argtypes = \[(.*?)\]\n" % name, src).group(1)
        assert [a.strip() for a in got.split(",")] == want, name
        assert '"%s"' % name in src
