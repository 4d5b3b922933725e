"""Host-side shape rule of the voxel encoder (no GPU): odd extents are accepted, an axis shorter than 4 is refused with a
ValueError before anything reaches the library."""
import pytest
import torch

from multimodal_eeg_fmri_amd import ops
import multimodal_eeg_fmri_amd.fmri_utils as Fm


@pytest.mark.parametrize("shape", [(2, 1, 91, 109, 91), (1, 1, 61, 73, 61), (3, 1, 64, 64, 33), (1, 1, 4, 4, 4),
                                   (4, 1, 16, 16, 24)])
def test_odd_and_even_extents_of_at_least_four_are_accepted(shape):
    ops.check_volume_shape(shape)
    ops.check_volume_shape(torch.Size(shape))


@pytest.mark.parametrize("shape", [(2, 1, 3, 16, 16), (2, 1, 16, 2, 16), (2, 1, 16, 16, 1), (1, 1, 0, 8, 8)])
def test_extents_below_four_are_refused(shape):
    with pytest.raises(ValueError, match=">= 4"):
        ops.check_volume_shape(shape)


def test_the_module_refuses_before_its_device_check():
    """the shape rule runs first: a CPU tensor with a bad shape gets the ValueError, not the missing-GPU error"""
    m = Fm.fMRIVolumeEncoder3D()
    with pytest.raises(ValueError, match=">= 4"):
        m(torch.zeros(1, 1, 8, 3, 8))
    with pytest.raises(ValueError, match="B, C, D, H, W"):
        ops.check_volume_shape((8, 8, 8))
