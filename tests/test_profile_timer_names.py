"""profiles/summarize_pmc.py::timer_name maps a profiler's kernel name to the timer name bench.py reports.  The inverse FFT kernel is
timed as k_node_fft (NODE = true) or k_rl_inverse (NODE = false), and NODE is the third template argument both in the nine-argument
names of the profiles recorded up to r06 and in today's six-argument names."""
import csv
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("(double const*, sx::Planes<double>, double const*, int const*, long const*, HIP_vector_type<double, 2u> const*, long const*, "
        "HIP_vector_type<double, 2u> const*, int const*, int, int, int, int, int, long, long, int, int, int, int, int, int, int, "
        "double const*, long, double const*, int, int)")
# <LOGL, ST, NODE, AT, FUSE, REG>: the library's demangled symbols
NEW = {
    "void sx::k_rl_inverse_fft<8, double, true, double, false, true>" + ARGS: "k_node_fft",
    "void sx::k_rl_inverse_fft<8, double, false, double, false, true>" + ARGS: "k_rl_inverse",
    "void sx::k_rl_inverse_fft<9, float, true, float, false, false>" + ARGS: "k_node_fft",
    "void sx::k_rl_inverse_fft<4, float, false, double, false, false>" + ARGS: "k_rl_inverse",
    "void sx::k_rl_inverse_fft<8, float, true, double, true, false>" + ARGS: "k_node_fft",
}


def _timer_name():
    spec = importlib.util.spec_from_file_location("summarize_pmc", os.path.join(ROOT, "profiles", "summarize_pmc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.timer_name


def test_recorded_nine_argument_names():
    """<LOGL, COPYOUT, NODE, ST, AT, HL, SETS, FUSE, REG>, as recorded in profiles/r06/branch_kernel_stats.csv"""
    timer_name = _timer_name()
    rows = [r["Name"] for r in csv.DictReader(open(os.path.join(ROOT, "profiles", "r06", "branch_kernel_stats.csv"))) if "k_rl_inverse_fft<" in r["Name"]]
    seen = {n.split("<")[1].split(">")[0]: timer_name(n) for n in rows}
    assert seen == {"8, 1, true, double, double, 0, 2, false, true": "k_node_fft", "8, 1, false, double, double, 0, 2, false, true": "k_rl_inverse"}, seen


@pytest.mark.parametrize("name", list(NEW))
def test_six_argument_names(name):
    assert _timer_name()(name) == NEW[name]


def test_other_kernels_keep_their_mapping():
    timer_name = _timer_name()
    assert timer_name("void sx::k_fl_forward_fft<8, double>(double const*)") == "k_fl_forward"
