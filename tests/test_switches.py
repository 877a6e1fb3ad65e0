"""The process-wide test / A-B switch type of the kernel launchers (markushgrapher_amd/csrc/mg_switch.h), checked on the CPU: the header is
plain C++17, so tests/switch_check.cpp includes it on its own, and every case runs in a fresh child process with a chosen environment
(a switch resolves the environment once per process)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAR = "MG_TEST_SWITCH"


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("switch_check") / "switch_check")
    cmd = ["g++", "-std=c++17", "-pthread", "-O1", "-I", os.path.join(ROOT, "markushgrapher_amd", "csrc"),
           os.path.join(ROOT, "tests", "switch_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout

    def run(case, want, env_value=None):
        env = {k: v for k, v in os.environ.items() if k != VAR}
        if env_value is not None:
            env[VAR] = env_value
        r = subprocess.run([exe, case, str(want)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        assert r.returncode == 0, (case, env_value, r.returncode, r.stdout)

    return run


def test_default_when_unset(check):
    check("get", 7)


@pytest.mark.parametrize("text,value", [("3", 3), ("0", 0), ("-1", -1)])
def test_environment_on_first_get(check, text, value):
    check("get", value, text)


def test_set_before_first_get_beats_environment(check):
    check("set_first", 5, "3")
    check("set_first", 5)


def test_set_after_get_wins(check):
    check("set_after", 3, "3")
    check("set_after", 7)


def test_sixteen_threads_see_one_value(check):
    check("threads", 3, "3")
    check("threads", 7)


@pytest.mark.parametrize("text,value", [(None, -1), ("0", 0), ("1", 1), ("2", -1), ("x", -1)])
def test_switch_with_its_own_accepted_values(check, text, value):
    """MG_ROWS_FT2's rule: only 0 or 1 count, anything else is the default."""
    check("parse", value, text)
