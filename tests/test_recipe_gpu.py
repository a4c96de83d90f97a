"""StepConfig.spatial_normalize / StepConfig.no_non_rigid_mask and the spatial-normalisation kernels on the MI355X (bodies:
tests/recipe_cases.py; the emulator runs the same cases in tests/test_recipe.py)."""
import pytest

import recipe_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_against_float64(name):
    C.check_forward_against_float64(name, "cuda")


@pytest.mark.parametrize("which", C.GRADS)
@pytest.mark.parametrize("name", C.NAMES)
def test_backward_against_float64(name, which):
    C.check_backward_against_float64(name, which, "cuda")


@pytest.mark.parametrize("name", C.NAMES)
def test_against_reference(name):
    C.check_against_reference(name, "cuda")


def test_reproducible_and_level_alone_equals_its_row():
    C.check_reproducible("cuda")


def test_levels_surface():
    C.check_levels_surface("cuda")


def test_entry_points_refuse_bad_tables():
    C.check_argument_errors("cuda")


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("recipe", ["a", "b", "c"])
def test_step_against_reference(recipe, use_graph):
    C.check_step_against_reference(recipe, use_graph, "cuda")


@pytest.mark.parametrize("deterministic", [False, True])
def test_step_forms_agree(deterministic, monkeypatch):
    """What tests/test_nets_gpu.py::test_step_forms_agree holds the default recipe to, with spatial_normalize.  (Inside the whole suite
    this test sits where the round-robin stream pool once made a trainer's Back2Future stream the capture stream itself:
    test_capture_stream_is_none_of_the_network_streams.)"""
    C.check_step_forms_agree(deterministic, monkeypatch, "cuda")


@pytest.mark.parametrize("use_graph", [False, True])
def test_loss_phase_on_two_streams_changes_no_bit(use_graph, monkeypatch):
    C.check_switch_changes_no_bit("loss_stream", use_graph, monkeypatch, "cuda")


@pytest.mark.parametrize("use_graph", [False, True])
def test_network_streams_change_no_bit(use_graph, monkeypatch):
    C.check_switch_changes_no_bit("net_streams", use_graph, monkeypatch, "cuda")


def test_config2_against_float64_oracle():
    C.check_config2_against_oracle("cuda")


def test_default_fields_change_no_bit(monkeypatch):
    C.check_explicit_defaults_change_no_bit("cuda")
    C.check_explicit_defaults_step("cuda", monkeypatch)


def test_capture_stream_is_none_of_the_network_streams(monkeypatch):
    """torch hands streams out of a pool of 32, round-robin, and torch.cuda.graph's default capture stream is one of them: a
    trainer's side streams can be that very stream.  The step's stream and a network's stream were then one, the per-stream
    weight-gradient queues merged (PoseNetB6 conv3 joined Back2Future's conv3a-c in one group launch) and the captured step differed
    from other trainers' in the last bit of those four gradients.  CCTrainer._capture_stream skips the streams already taken."""
    C.check_capture_stream(monkeypatch, "cuda")
