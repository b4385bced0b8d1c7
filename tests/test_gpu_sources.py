"""A source is a source, on the GPU: the cases of ``test_sources_cpu.py`` (``source_cases``) with ``device=0`` -- the
container functions go through ``fra_decode_device_*``, the GeoTIFF functions through the array entries -- and every
result equal to what ``device=None`` gives."""
import pytest

import source_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    fix = SC.build(tmp_path_factory.mktemp("gpu_sources"))
    return SC.results(fix, 0), SC.results(fix, None)


def test_every_case_ran(both):
    assert sorted(both[0]) == sorted(SC.CASES)
    SC.check_windows(both[0])


@pytest.mark.parametrize("name,case", SC.CASES)
def test_container_and_geotiff_agree_on_the_gpu_and_with_the_host(both, name, case):
    dev, host = both
    a, b = dev[name, case]
    SC.same(a, b, f"{name}, {case}")
    SC.same(a, host[name, case][0], f"{name}, {case}: device against host")
