"""What pwr_set_option / pwr_get_option answer, probed key by key: shared by scripts/gen_option_fixture.py, which records
the answers of one build of the library in tests/golden/pwr_options.json, and by the tests that replay that record against
the library in the tree (test_pwr_options.py on the host, test_gpu_pwr_options.py after the first device call)."""
import ctypes
import hashlib
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "pwr_options.json")

# every key pwr_set_option or pwr_get_option knew when the record was made, and two that neither knows
KEYS = ["window", "profile", "spec_len", "fill", "stall_test", "evcap", "force64", "ptrace", "slack", "fill_epoch", "trace_epoch",
        "onewg", "fill_lds", "onewg_lds", "seg_rows", "seg_align", "seg_max", "seg_budget", "plan_slack", "hard_rows", "hard_up_pm",
        "hard_down_pm", "check_in_trace", "trace_prior", "plan_len", "plan_gate_rel", "spec_inorder", "fail_stops",
        "plan_evrate_x100", "plan_ahead", "seg_balance", "seg_minrows", "src_start", "warm_adapt", "warm_down_pm", "warm_up_pm",
        "warm_min_pct", "warm_pct", "wave_cols", "waves",
        "hard_marked", "hard_fills", "hard_refail", "evrate_x100", "warm_now", "host_enqueue_us", "host_wait_us",
        "threads", "nonsense"]

# on both sides of every bound of the setter the record was made from
PROBES = [-1, 0, 1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 32, 64, 128, 129, 256, 257, 1000, 1001, 1024, 1025, 10000, 10001, 16383, 16384,
          32767, 32768, 100000, 100001, 1000000, 1000001, 100000000, 100000001, 2147483647]

# The keys that could be set and not read when the record was made.  A library that reads them too is accepted (the tests
# then ask for the value last set); they stay out of the digests, so that a record made from such a library differs from
# this one in their own `get` entries alone.
WRITE_ONLY_WHEN_RECORDED = ["stall_test", "evcap", "fill_epoch", "trace_epoch", "fill_lds", "onewg_lds", "seg_align", "wave_cols"]

ERR_ARG = -1
DEVICE_CASE, DEVICE_BANDWIDTH = "edge_mixed_case", 8


def create(lib, rows, bandwidth):
    h = ctypes.c_void_p()
    rc = lib.pwr_create(ctypes.byref(h), len(rows), len(rows[0]), b"".join(rows), bandwidth, 0)
    assert rc == 0, rc
    return h


def get(lib, h, key):
    """[return code, value]; the value is null when the call failed"""
    v = ctypes.c_long(0)
    rc = lib.pwr_get_option(h, key.encode(), ctypes.byref(v))
    return [rc, v.value if rc == 0 else None]


def set_(lib, h, key, value):
    return lib.pwr_set_option(h, key.encode(), value)


def others(lib, h, key):
    return [[k] + get(lib, h, k) for k in KEYS if k != key]


HOST_ROWS = [b"acgt", b"ac-t"]


def probe_host(lib, key):
    """Every probe value, each on a fresh context that never touches the device: the codes of set and get and the value get
    gives, per probe, and one digest of what every other key gives before and after each of them.  For the tests, second:
    per probe, the same key's get before the set and whether the other keys that the digest leaves out gave the same
    before and after."""
    rec, extra, seen = {"set": [], "get_rc": [], "get": []}, [], []
    for value in PROBES:
        h = create(lib, HOST_ROWS, 1000)
        fresh = get(lib, h, key)
        before = others(lib, h, key)
        rec["set"].append(set_(lib, h, key, value))
        rc, v = get(lib, h, key)
        rec["get_rc"].append(rc)
        rec["get"].append(v)
        after = others(lib, h, key)
        lib.pwr_destroy(h)
        seen.append([[e for e in o if e[0] not in WRITE_ONLY_WHEN_RECORDED] for o in (before, after)])
        left_out = [[e for e in o if e[0] in WRITE_ONLY_WHEN_RECORDED] for o in (before, after)]
        extra.append((fresh, left_out[0] == left_out[1]))
    rec["others"] = hashlib.sha256(json.dumps(seen).encode()).hexdigest()[:16]
    return rec, extra


def probe_defaults(lib):
    h = create(lib, HOST_ROWS, 1000)
    d = {k: get(lib, h, k) for k in KEYS}
    lib.pwr_destroy(h)
    return d


def lowest_accepted(host, key):
    """the lowest probe value the host part's set accepted for this key, or null"""
    ok = [v for v, rc in zip(PROBES, host[key]["set"]) if rc == 0]
    return min(ok) if ok else None


def device_context(lib, rows):
    """a context after its first device call, as the device part asks: trim_ends, realign_row(0)"""
    h = create(lib, rows, DEVICE_BANDWIDTH)
    assert lib.pwr_trim_ends(h) == 0
    assert lib.pwr_realign_row(h, 0) == 0
    return h
