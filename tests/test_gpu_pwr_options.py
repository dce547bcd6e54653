"""After the first device call, pwr_get_option / pwr_set_option answer what the device part of tests/golden/pwr_options.json
records (scripts/gen_option_fixture.py): which keys can still be read, and which lock."""
import json

import pytest

import pwr_option_probe as pp
from conftest import golden_input, split_rows


@pytest.mark.gpu
def test_options_after_the_first_device_call_answer_as_recorded():
    from repeatresolver_amd import _lib
    lib = _lib.load()
    with open(pp.FIXTURE) as f:
        rec = json.load(f)["device"]
    h = pp.device_context(lib, split_rows(golden_input(pp.DEVICE_CASE)))
    bad = []
    for k in pp.KEYS:
        want = rec[k]
        rc, v = pp.get(lib, h, k)
        # (a key the record could set and not read may be read now; it is then set to what it gave, as every readable key is)
        if rc != want["get"] and not (k in pp.WRITE_ONLY_WHEN_RECORDED and want["get"] == pp.ERR_ARG and rc == 0):
            bad.append((k, "get", rc, want["get"]))
        if rc != 0:
            v = want["set_to"]
        got = None if v is None else pp.set_(lib, h, k, v)
        if got != want["set"]:
            bad.append((k, "set", v, got, want["set"]))
    lib.pwr_destroy(h)
    assert not bad, bad
