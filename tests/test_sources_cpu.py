"""A source is a source, on the host (no GPU needed): every windowed operation gives the same result over a streaming
container -- as a file and as bytes -- and over the GeoTIFF written from that container's pixels, for the whole raster,
a pixel window across tile corners and a bbox; and a GeoTIFF's own nodata tag, taken when no value is given, gives what
the container gives with that value.  ``source_cases`` holds the fixture and the cases."""
import pytest

import source_cases as SC


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    fix = SC.build(tmp_path_factory.mktemp("sources"))
    return fix, SC.results(fix, None)


def test_every_case_ran(host):
    assert sorted(host[1]) == sorted(SC.CASES)
    SC.check_windows(host[1])


@pytest.mark.parametrize("name,case", SC.CASES)
def test_container_and_geotiff_agree(host, name, case):
    a, b = host[1][name, case]
    SC.same(a, b, f"{name}, {case}")


def test_the_fixture_is_what_the_issue_names(host):
    fix, _ = host
    assert fix.plain.shape == (3, 96, 130) and fix.plain.dtype == "uint16"
    assert (fix.plain[2] == fix.nodata).sum() > fix.plain[2].size // 2 and len(fix.targets) == 3
