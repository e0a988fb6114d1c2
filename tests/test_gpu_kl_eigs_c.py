"""tests/c/kl_matern_smoke.c: the device Matern eigensolver called from plain C through include/pmc.h"""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_c_caller():
    r = subprocess.run(["make", "-C", ROOT, "test-kl-matern"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "c", "bin", "kl_matern_smoke")], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("kl_matern_smoke OK"), r.stdout + r.stderr
