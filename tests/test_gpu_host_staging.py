"""The host entry points' staging (3dworld_amd/csrc/terra_stage.hpp) on the MI355X: host form against device form on arrays the test uploads itself, untouched
padding, a scratch that is regrown, the empty batch -- the cases of tests/host_staging_cases.py, as test_host_staging_emul.py runs them on the emulator."""
import pytest

import host_staging_cases as hsc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("opt", hsc.OPTS)
@pytest.mark.parametrize("entry", hsc.ENTRIES)
def test_host_form_equals_device_form(pkg, gpu, entry, opt):
    hsc.run_forms(pkg, gpu, entry, opt)


@pytest.mark.parametrize("entry", hsc.ENTRIES)
def test_scratch_regrowth(pkg, gpu, entry):
    hsc.run_regrowth(pkg, gpu, entry)


@pytest.mark.parametrize("entry", hsc.ENTRIES)
def test_empty_batch(pkg, gpu, entry):
    hsc.run_empty(pkg, gpu, entry)
