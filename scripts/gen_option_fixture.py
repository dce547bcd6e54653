"""Records what pwr_set_option / pwr_get_option answer in tests/golden/pwr_options.json (tests/pwr_option_probe.py has the
keys, the probe values and the probes themselves; tests/test_pwr_options.py and tests/test_gpu_pwr_options.py replay the record).

The record is made from a build of the commit BEFORE a change to the option code, never from the code under test:
    python scripts/dev/with_lib.py <that build's libpwr.so> scripts/gen_option_fixture.py [--host-only] [--out FILE]

Host part (no GPU): for every key and probe value, on a fresh context, the code of set and the code and value of get afterwards;
per key a digest of what every other key gives before and after each probe; and every key's get on a fresh context (the defaults).
Device part (one short GPU run; left as it is in FILE with --host-only): edge_mixed_case at bandwidth 8 after trim_ends and
realign_row(0): the code of get for every key, and the code of set to the value get gave (for a key that cannot be read: to the
lowest value the host part accepted) -- which keys lock at the first device call."""
import argparse
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pwr_option_probe as pp  # noqa: E402
from repeatresolver_amd import _lib  # noqa: E402


def device_part(lib, host):
    with gzip.open(os.path.join(pp.GOLDEN, pp.DEVICE_CASE + ".in.gz"), "rb") as f:
        rows = f.read().split(b"\n")[:-1]
    h = pp.device_context(lib, rows)
    out = {}
    for k in pp.KEYS:
        rc, v = pp.get(lib, h, k)
        low = None if rc == 0 else pp.lowest_accepted(host, k)           # ("set_to" null: to the value get gave)
        v = v if rc == 0 else low
        out[k] = {"get": rc, "set_to": low, "set": None if v is None else pp.set_(lib, h, k, v)}
    lib.pwr_destroy(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=pp.FIXTURE)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    rec = {"keys": pp.KEYS, "probes": pp.PROBES, "write_only": pp.WRITE_ONLY_WHEN_RECORDED,
           "defaults": pp.probe_defaults(lib),
           "host": {k: pp.probe_host(lib, k)[0] for k in pp.KEYS}}
    if a.host_only:
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
            if "device" in old:
                rec["device"] = old["device"]
    else:
        rec["device"] = device_part(lib, rec["host"])
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in rec.items()) + "\n}\n")
    print(f"{a.out}: {len(pp.KEYS)} keys x {len(pp.PROBES)} probes" + ("" if a.host_only else ", device part"))


if __name__ == "__main__":
    main()
