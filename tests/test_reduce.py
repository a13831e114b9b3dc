"""The cross-locus reduction through its probe (gph_debug_reduce_) on the host builds: the serial loop the host engine sums with,
called by the engine and by the probe alike (csrc/gph_backend.h: reduce_serial).  References (a) integer sums, (b) math.fsum with
d = L, (d) planted extremes and special values, (e) what must stay unwritten, (f) launches back to back, and the refusals -- the
bodies are in reduce_util.py and run again on the MI355X (test_reduce_gpu.py), where the documented shape (c) joins them.
Every locus count of the device tests runs here too: the serial loop takes well under a second for the largest."""
import pytest

import reduce_util as U


@pytest.fixture(scope="module")
def lib128():
    return U.host_library()


@pytest.fixture(scope="module")
def lib384():
    return U.host_library(wide=True)


def test_constants(lib128, lib384):
    a, b = U.constants(lib128), U.constants(lib384)
    assert (a.cols, b.cols) == (128, 384)                  # which is what makes them the libraries these tests want
    for i in (a, b):
        assert i.stride == 3 * i.cols + 8 and i.row == 2 * i.stride and i.subs == 0 and i.ticket == 0
        assert i.poison >> 51 == 0xFFF and i.poison & ((1 << 51) - 1) != 0        # a quiet NaN with a payload


def test_refusals(lib128, lib384):
    U.check_refusals(lib128)
    U.check_refusals(lib384)


@pytest.mark.parametrize("ncols", U.WIDTHS_0)
def test_section_0(lib128, ncols):
    print(f"section 0, {ncols} columns: worst |row - fsum| / bound {U.check_width(lib128, 0, ncols, 1000 + ncols):.3f}")


@pytest.mark.parametrize("ncols", U.WIDTHS_128)
def test_section_1(lib128, ncols):
    print(f"section 1, {ncols} columns: worst |row - fsum| / bound {U.check_width(lib128, 1, ncols, 2000 + ncols):.3f}")


@pytest.mark.parametrize("ncols", U.WIDTHS_384)
def test_section_1_wide_rows(lib384, ncols):
    print(f"section 1, {ncols} columns: worst |row - fsum| / bound {U.check_width(lib384, 1, ncols, 3000 + ncols):.3f}")


# the large counts, two tests a case: the references (36 million numbers through math.fsum at the largest) take a second or two each
@pytest.mark.parametrize("L", U.LOCI_LARGE)
@pytest.mark.parametrize("sec,ncols", U.LARGE_128)
def test_many_loci_sums(lib128, sec, ncols, L):
    U.check_floats(lib128, sec, ncols, L, 4001 + L)


@pytest.mark.parametrize("L", U.LOCI_LARGE)
@pytest.mark.parametrize("sec,ncols", U.LARGE_128)
def test_many_loci_integers_and_extremes(lib128, sec, ncols, L):
    U.check_integers(lib128, sec, ncols, L, 4000 + L)
    U.check_extremes(lib128, sec, ncols, L, 4002 + L)


@pytest.mark.parametrize("L", U.LOCI_LARGE)
@pytest.mark.parametrize("sec,ncols", U.LARGE_384)
def test_many_loci_sums_wide_rows(lib384, sec, ncols, L):
    U.check_floats(lib384, sec, ncols, L, 5001 + L)


@pytest.mark.parametrize("L", U.LOCI_LARGE)
@pytest.mark.parametrize("sec,ncols", U.LARGE_384)
def test_many_loci_integers_and_extremes_wide_rows(lib384, sec, ncols, L):
    U.check_integers(lib384, sec, ncols, L, 5000 + L)
    U.check_extremes(lib384, sec, ncols, L, 5002 + L)


@pytest.mark.parametrize("ncols", (16, 26, 110))
def test_both_sections_in_one_call(lib128, ncols):
    for L in (1, 257, 2049):
        U.check_fused(lib128, ncols, L, 6000 + L)


def test_both_sections_in_one_call_wide_rows(lib384):
    for L in (257, 2049):
        U.check_fused(lib384, 278, L, 6100 + L)
