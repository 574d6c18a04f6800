"""What the CPU tests of the three rigs of a batch - sensors, cameras, zones - share: the text of the steps host_batch_rig.inc writes
once, cut out function by function for the source-reading assertions of tests/test_world_batch_{sensors,cameras,zones,rigs}_host.py, and
the cases of the one test of a rig's plan."""
from tests import batch_query_device_cases as QD
from tests import batch_sensor_cases as SC
from tests import batch_zone_cases as ZC
from tests.util import read

RIG_FILES = {"sensors": "host_batch_sensor.inc", "cameras": "host_batch_camera.inc", "zones": "host_batch_zone.inc"}


def rig_source():
    return read("mgf_amd", "csrc", "host_batch_rig.inc")


def _cut(src, start, end):
    return src[src.index(start):src.index(end)]


def set_args_step():
    return _cut(rig_source(), "static mgf_status batch_rig_set_args(", "// what a record of a rig")


def ref_check_step():
    return _cut(rig_source(), "static mgf_status batch_rig_ref_check(", "// The records become the rig")


def plan_step():
    return _cut(rig_source(), "static void batch_rig_plan(", "// Sections onto the device")


def upload_step():
    return _cut(rig_source(), "static mgf_status batch_rig_upload(", "// The rig onto the device")


def up_step():
    return _cut(rig_source(), "static mgf_status batch_rig_up(", "// What a cast or a read of a rig refuses")


def args_steps():
    src = rig_source()
    return src[src.index("static mgf_status batch_rig_handle("):]


def stale_step():
    host = read("mgf_amd", "csrc", "host_batch.inc")
    return _cut(host, "static void batch_rigs_stale(", 'extern "C" mgf_status mgf_batch_add_bodies(')


def set_call_with_plan(body, call):
    """a set function's text with the shared plan step where it is called: what "every refusal precedes the first change of the rig"
    is read in"""
    at = body.index(call)
    return body[:at] + plan_step() + body[at + len(call):]


def assert_the_read_and_cast_refusals(args, own, null_msg=None):
    """an args function of a rig: the handle, then `own` and the sign of cap in the given order, then - batch_rig_fits - the capacity
    ahead of the NULL output; nothing of it looks at a device"""
    steps = args_steps()
    order = [args.index(s) for s in ["batch_rig_handle(b)"] + own + ["batch_rig_fits(*n, cap, "]]
    assert order == sorted(order), (own, order)
    if null_msg:
        assert null_msg in args[args.index("batch_rig_fits("):]
    fits = steps[steps.index("static mgf_status batch_rig_fits("):]
    assert '"batch is NULL"' in steps and '"cap is negative"' in steps
    assert fits.index("MGF_ERR_CAPACITY") < fits.index("null_msg);") < fits.index("return MGF_OK;")
    assert 'const char* null_msg = "NULL argument"' in fits
    for text in (args, steps):
        assert "ctx_bind" not in text and "<<<" not in text


def plan_cases():
    """(name, whose, world, K, counts): the sensors' four and the zones' seven"""
    twin, pile = SC.twin_scenes(), QD.pile_scenes()
    cases = [("worlds of 0, 1, 256, 257 and 600", "sensors", SC.plan_worlds(), len(SC.PLAN_COUNTS), list(SC.PLAN_COUNTS)),
             ("the same reversed", "sensors", SC.plan_worlds()[::-1], len(SC.PLAN_COUNTS), list(SC.PLAN_COUNTS)),
             ("twin", "sensors", SC.twin_layout(twin)["world"], len(twin), [0, 1, 257]),
             ("pile", "sensors", SC.pile_layout(pile)["world"], len(pile), [2, 42, 60, 0, 320])]
    cases += [(name, "zones", ZC.plan_worlds(counts), len(counts), list(counts)) for name, counts in ZC.PLAN_CASES]
    return cases


PLAN_IDS = ["sensors-0", "sensors-1", "sensors-2", "sensors-3"] + [f"zones-{i}" for i in range(len(ZC.PLAN_CASES))]

