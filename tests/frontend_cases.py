"""What the front end's host code (csrc/frontend_api.hip) fixes when it is compiled, read from the source the way capacity_cases.py
reads the kernels' caps: a changed constant then fails the tests sized by it instead of silently un-testing what they are for."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONTEND_API = os.path.join(ROOT, "herro_amd", "csrc", "frontend_api.hip")


def slice_records() -> int:
    """records per turn of the slice loops of herro_extend_overlaps and herro_aligned_dev_mirror"""
    m = re.search(r"constexpr uint32_t SLICE = 1u << (\d+);", open(FRONTEND_API).read())
    assert m, "SLICE is no longer a constexpr of frontend_api.hip"
    return 1 << int(m.group(1))
