import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")
    config.addinivalue_line("markers", "default_policy: LU tests that run under the default policy (tests/test_gpu_lu.py)")


@pytest.fixture(scope="session")
def oracle():
    from oracle import pyoracle
    pyoracle.build(ref=os.path.isdir("/root/reference"))
    return pyoracle.Oracle()


@pytest.fixture(scope="session")
def live_ref(oracle):
    from oracle import pyoracle
    if not pyoracle.ref_available() or os.environ.get("IPXK_REF") == "replay":
        return None
    return pyoracle.Ref()


@pytest.fixture
def ref(live_ref, request):
    """The reference's own objects: live where oracle/_ref is built, else their recorded answers
    (tests/refcalls.py; IPXK_REF=record re-records them from the live build)."""
    import refcalls
    path, key = refcalls.path_for(request.node.nodeid), refcalls.test_key(request.node.nodeid)
    if live_ref is None:
        log = refcalls.Log.load(path, key)
        if log is None:
            pytest.skip("oracle/_ref not built and no recorded answers for this test in %s (answers over %d KB "
                        "are not recorded)" % (os.path.relpath(path, ROOT), refcalls.MAX_BYTES >> 10))
        yield refcalls.replayer(log)
    elif os.environ.get("IPXK_REF") == "record":
        log = refcalls.Log()
        yield refcalls.recorder(live_ref, log)
        if request.node.rep_call.passed:
            log.save(path, key)
    else:
        yield live_ref


@pytest.hookimpl(hookwrapper=True)
def pytest_runtest_makereport(item, call):
    rep = (yield).get_result()
    if rep.when == "call":
        item.rep_call = rep
