"""CPU: pt_queue_plan.h, the integer arithmetic every hot kernel gets its work through (which rays a traversal wave claims, where hit
records go in the striped shade queues, path id <-> (sample, pixel)), swept by the stand-alone sanitizer driver (`host_sanitize queues`,
AddressSanitizer + UBSan, `make -C path_tracer_amd/csrc host-asan`) over the ray counts where a regime changes: 1..4200, every
2^k - 1, 2^k, 2^k + 1 below 2^29 and log-uniform ones, under every grid, workgroup shape, chunk divisor and taper the launchers use.
The driver recomputes every expectation in 64-bit arithmetic or from the other side of a producer / consumer pair and exits nonzero
on a mismatch; this test also holds it to having looked at something for every property."""
import json

from test_host_sanitizer import _run, exe  # noqa: F401  (exe: the fixture that builds the driver)

N_COUNTS_MIN = 4200 + 80            # the exhaustive range, the powers of two and their neighbours; the log-uniform ones may repeat some
CONFIGS = 7 * 3 * 2 * 2             # grids x waves per workgroup x chunk divisors x tapers


def test_queue_arithmetic_properties(exe):
    res = json.loads(_run([exe, "queues", "1"]).strip().split("\n")[-1])
    assert res["failures"] == 0, res
    # P1: claims partition the queue
    assert res["p1_cases"] >= N_COUNTS_MIN * CONFIGS and res["p1_cases"] % CONFIGS == 0, res
    assert res["p1_static"] >= res["p1_cases"] and res["p1_chunks"] >= 10 * res["p1_cases"], res
    # P2: striped regions (four capacities per ray count; refusals among them)
    assert res["p2_cases"] * CONFIGS == res["p1_cases"] and res["p2_regions"] > res["p2_cases"] and res["p2_slots"] >= 16 * res["p2_cases"], res
    assert res["p2_refused"] >= res["p2_cases"], res
    # P3: region_size over 31 producer counts and two minimum sizes
    assert res["p3_cases"] >= res["p2_cases"] * 31 * 2, res
    # P4: fastdiv: 1..4096, the powers of two and their neighbours, 4000 random divisors; at least forty dividends each
    assert res["p4_divisors"] >= 4096 + 90 + 4000 and res["p4_divisions"] >= 40 * res["p4_divisors"], res
    # P5: 73 sample counts x 8 pixel counts, less the batches the planner refuses (2^29 paths or more: 2 073 600 pixels from 259 samples on, none here)
    assert res["p5_cases"] == 73 * 8 and res["p5_ids"] >= 10_000_000, res

