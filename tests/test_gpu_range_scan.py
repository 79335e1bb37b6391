"""dlsm_range_scan under a context: the host form honours the context's
DLSM_OPT_FAULT_INJECT and runs as before once it is cleared.  (The scan itself
touches no device; the context is what needs one.)"""
import pytest

import dlsm_amd
from range_scan_cases import two_files
from test_range_scan_host import run_case, scan

pytestmark = pytest.mark.gpu


def test_fault_injection_reaches_the_host_form(gpu):
    c = dict(two_files(), starts=[b"", b"0000000000000007"], snapshot=100, limit=4)
    gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 4)
    try:
        with pytest.raises(dlsm_amd.DlsmError) as e:
            scan(c, [512, 512, 16], ctx=gpu)
        assert e.value.status == -4
    finally:
        gpu.set_option(dlsm_amd.OPT_FAULT_INJECT, 0)
    run_case(c, gpu)
