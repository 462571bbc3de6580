"""GPU: the view passes (render_map, render_mesh, multiview_support, fuse_tsdf and their C entry points) give the bytes
they gave before they were folded onto csrc/view_dev.h and cons_planes.h.

tests/golden/view_family_digests.json holds the SHA-256 of every output and of every input array of the cases of
tools/record_view_digests.py, recorded with the library of the commit before the fold.  The digests are recomputed
here; a changed input digest (numpy, the scene modules) is reported apart from a changed output digest (the kernels)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def digests(dev):
    spec = importlib.util.spec_from_file_location("record_view_digests", os.path.join(ROOT, "tools", "record_view_digests.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(rec.GOLDEN) as fh:
        return json.load(fh), rec.compute(dev)


def changed(want, got):
    return sorted(k for k in set(want) | set(got) if want.get(k) != got.get(k))


def test_inputs_are_the_recorded_ones(digests):
    want, got = digests
    assert len(want["inputs"]) >= 10
    assert changed(want["inputs"], got["inputs"]) == [], "the scenes differ from the recorded ones: not a kernel change"


def test_outputs_are_the_recorded_bytes(digests):
    want, got = digests
    bad_inputs = changed(want["inputs"], got["inputs"])
    assert len(want["outputs"]) >= 40
    assert changed(want["outputs"], got["outputs"]) == [], f"outputs changed (inputs changed: {bad_inputs or 'none'})"


def test_the_consistency_cases_tell_their_arguments_apart(digests):
    """On the shared scene the neighbour table and the threshold change the result, in the hand case the conflict limit
    does: these digests test the branches they were chosen for."""
    got = digests[1]["outputs"]
    assert len({got[f"consistency shared {k}"] for k in ("all", "table", "all no threshold")}) == 3
    assert len({got[f"consistency hand{k}"] for k in ("", " views 0 limit 0", " views 0 no limit")}) == 3


def test_infinite_principal_point_through_the_c_entries(digests):
    """m3_render_map and m3_raster_mesh return M3_OK (0) and draw the background; m3_consistency and m3_tsdf_integrate
    return M3_ERR_INVALID_ARG (-1) and write nothing: outputs and workspace keep their fill (part of the digest)."""
    want, got = digests
    for name, rc in (("m3_render_map", 0), ("m3_raster_mesh", 0), ("m3_consistency", -1), ("m3_tsdf_integrate", -1)):
        key = f"{name} cx=inf"
        assert got["outputs"][key].split()[0] == str(rc) and got["outputs"][key] == want["outputs"][key]
    assert got["outputs"]["m3_render_map cx=inf"] == got["outputs"]["m3_raster_mesh cx=inf"]      # both: the background
