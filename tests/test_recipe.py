"""StepConfig.spatial_normalize / StepConfig.no_non_rigid_mask and the spatial-normalisation kernels on the x86 emulation build of the
kernel sources (bodies: tests/recipe_cases.py; the same cases run on the MI355X in tests/test_recipe_gpu.py)."""
import pytest

import recipe_cases as C
from hipemu.emu import emulated_engine


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_against_float64(name):
    with emulated_engine():
        C.check_forward_against_float64(name, "cpu")


@pytest.mark.parametrize("which", C.GRADS)
@pytest.mark.parametrize("name", C.NAMES)
def test_backward_against_float64(name, which):
    with emulated_engine():
        C.check_backward_against_float64(name, which, "cpu")


@pytest.mark.parametrize("name", C.NAMES)
def test_against_reference(name):
    with emulated_engine():
        C.check_against_reference(name, "cpu")


def test_reproducible_and_level_alone_equals_its_row():
    with emulated_engine():
        C.check_reproducible("cpu")


def test_levels_surface():
    with emulated_engine():
        C.check_levels_surface("cpu")


def test_entry_points_refuse_bad_tables():
    with emulated_engine():
        C.check_argument_errors("cpu")


@pytest.mark.slow
@pytest.mark.parametrize("recipe", ["a", "b"])
def test_step_against_reference(recipe):
    """one eager step per recipe: what the emulator suite can afford (all three recipes, captured too, on the MI355X)"""
    with emulated_engine():
        C.check_step_against_reference(recipe, False, "cpu")


def test_config2_against_float64_oracle():
    with emulated_engine():
        C.check_config2_against_oracle("cpu")


def test_default_fields_change_no_bit():
    with emulated_engine():
        C.check_explicit_defaults_change_no_bit("cpu")
