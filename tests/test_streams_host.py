"""not-gpu: herro_set_stream where there is no device (include/herro_amd.h, "Run all subsequent work of this context ...").  A device-free
context has no stream: NULL and any other value return HERRO_OK, make no HIP call and change nothing that can be observed — the job the
context builds afterwards is the job it built before, array for array.  A NULL context is HERRO_E_INVALID.  What a stream switch means on
the device is tests/test_gpu_streams.py's."""
import numpy as np

import aligned_dev_cases as AC
import build_cases as BC
from herro_amd import api


def _codes():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "herro_amd.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(HERRO_E_[A-Z_]+)\s+\(?(-?\d+)\)?", hdr)}


def _arrays(c, case):
    sb, W, rids, rows, aln_off, cigars = case
    job = c.create_job(rids, rows, aln_off, cigars, W)
    try:
        return {k: (v.dtype, v.tobytes()) for k, v in c.job_arrays(job).items()}, job.skipped(), job.n_windows
    finally:
        job.close()


def test_a_device_free_context_takes_any_stream_and_stays_as_it_was():
    case = BC.hand_case(AC.HAND_W)
    sb = case[0]
    c = api.HostContext((sb.off[1:] - sb.off[:-1]).astype(np.uint32))
    try:
        before = _arrays(c, case)
        assert before[2] > 0
        for s in (None, 0, 0x1000, None, 0x1000, 0x1000, 0x2000, 0):
            assert c._l.herro_set_stream(c.h, s) == 0, s
            c.set_stream(s)                                  # the wrapper: no exception
            assert c.last_error() == ""
            assert _arrays(c, case) == before, s
        assert c._l.herro_synchronize(None) == _codes()["HERRO_E_INVALID"]
    finally:
        c.close()


def test_a_null_context_is_invalid():
    L = api.lib()
    inval = _codes()["HERRO_E_INVALID"]
    assert inval == -1
    assert L.herro_set_stream(None, None) == inval
    assert L.herro_set_stream(None, 0x1000) == inval
