"""Host-side test of tests/gpu_child.py's run_child over trivial scripts: what every GPU job's result and failure report goes
through.  No GPU, no library."""
import subprocess

import pytest

from gpu_child import run_child


def test_a_failing_child_raises_with_its_stderr_tail():
    with pytest.raises(AssertionError, match="the reason on stderr"):
        run_child('import sys\nprint("RESULT {}")\nsys.stderr.write("the reason on stderr\\n")\nsys.exit(3)')
    with pytest.raises(AssertionError, match="done"):                                          # an "ok" child that does not say so
        run_child('print("done")', ok=True)
    assert "ok 7" in run_child('print("ok 7")', ok=True)


def test_the_last_result_line_is_returned():
    assert run_child('print("RESULT [1]")\nprint("noise")\nprint("RESULT {\\"n\\": 2}")\nprint("more")') == {"n": 2}


def test_env_and_args_reach_the_child():
    script = 'import os\nfrom gpu_child import emit, job_args\nemit(dict(knob=os.environ.get("SCS_TEST_KNOB"), home=os.environ.get("HOME"), args=job_args()))'
    assert run_child(script, dict(cov=2.0), env=dict(SCS_TEST_KNOB="12")) == dict(knob="12", home=None, args=dict(cov=2.0))


def test_a_child_past_its_timeout_raises():
    with pytest.raises(subprocess.TimeoutExpired):
        run_child("import time\ntime.sleep(5)", timeout=1)
