"""hpgv_run_set_output_compression: the setter alone (no device): the two modes are taken, anything else is refused and the
setting stays; and the bound callers size their buffers with."""
import ctypes as C
from importlib import import_module

import pytest

from helpers import hpgv

OUT_PLAIN, OUT_BGZF = 0, 1


@pytest.fixture(scope="module")
def host():
    hpgv.build()
    return C.CDLL(import_module("hpg-variant_amd._build").HOSTLIB)


def test_unknown_mode_is_refused_and_the_setting_stays(host):
    text = open(import_module("hpg-variant_amd._build").ROOT + "/include/hpgv_host.h").read()
    assert "HPGV_OUT_PLAIN = 0, HPGV_OUT_BGZF = 1" in text
    assert host.hpgv_run_set_output_compression(OUT_BGZF) == hpgv.OK
    for bad in (7, -1, 2):
        assert host.hpgv_run_set_output_compression(bad) == hpgv.ERR_INVALID
    # what a refused call left: still bgzip (a filter run without any filter fails before it writes, whatever the mode, so the
    # mode is read back through the setter's own contract: setting it again succeeds, and plain restores the default)
    assert host.hpgv_run_set_output_compression(OUT_BGZF) == hpgv.OK
    assert host.hpgv_run_set_output_compression(OUT_PLAIN) == hpgv.OK
    assert host.hpgv_run_set_output_compression(7) == hpgv.ERR_INVALID


def test_deflate_bound_covers_stored_members():
    L = hpgv.load()
    # a stored member is its text and 31 bytes; every segment may end in a short block of its own
    assert L.hpgv_bgzf_deflate_bound(0, 0) == 0
    assert L.hpgv_bgzf_deflate_bound(1, 1) >= 1 + 31
    assert L.hpgv_bgzf_deflate_bound(65280, 1) >= 65280 + 31
    assert L.hpgv_bgzf_deflate_bound(65281, 1) >= 65281 + 2 * 31
    assert L.hpgv_bgzf_deflate_bound(10 * 65280, 256) >= 10 * 65280 + (10 + 255) * 31
    assert L.hpgv_bgzf_deflate_scratch_bytes(10 * 65280, 3) >= 10 * 65280
