import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")
    config.addinivalue_line("markers", "ref: needs the compiled reference in oracle/_ref")


@pytest.fixture(scope="session")
def oracle():
    from oracle_lib import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def ref():
    """The compiled reference where oracle/_ref is built (with RSX_REF_RECORD=<file.npz>
    its answers are recorded into that file); elsewhere its stored answers
    (tests/ref_vectors.py, tests/golden/ref_vectors.json.gz)."""
    from oracle_lib import Ref
    import ref_vectors
    if not Ref.available():
        yield ref_vectors.StoredRef()
        return
    r = Ref()
    path = os.environ.get("RSX_REF_RECORD")
    if not path:
        yield r
        return
    rec = ref_vectors.RecordingRef(r, path)
    yield rec
    rec.save()
