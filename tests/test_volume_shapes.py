"""Host-side shape and width rules of the voxel encoder (no GPU): odd extents are accepted, an axis shorter than 4 is
refused with a ValueError before anything reaches the library; so is a channel width the kernels cannot run."""
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


@pytest.mark.parametrize("widths", [(32, 64, 128), (16, 32, 96), (32, 32, 64), (16, 16, 16), (64, 96, 160), (32, 64, 1024)])
def test_widths_of_16_or_a_multiple_of_32_are_accepted(widths):
    ops.check_volume_widths(widths)
    m = Fm.fMRIVolumeEncoder3D(widths=widths)
    assert [m.conv_layers[i].out_channels for i in (0, 5, 10)] == list(widths)
    assert m.output_proj[2].in_features == widths[2]


@pytest.mark.parametrize("widths", [(32, 48, 128), (32, 64, 100), (48, 64, 128), (32, 64, 48), (8, 64, 128), (32, 24, 128),
                                    (32, 64, 0), (32, 64, -32), (32, 64, 1056), (32, 64), (32, 64, 128, 256), (32.0, 64, 128),
                                    None])
def test_other_widths_are_refused_with_the_accepted_set_in_the_message(widths):
    """48 is a multiple of 16 (what weight images are padded to) but not of the 32-channel LDS chunk; 100 is not a multiple
    of 8; 8 and 24 are below / off the 16-channel chunk: ValueError at construction, naming the rule"""
    with pytest.raises(ValueError, match="16 or a multiple of 32"):
        ops.check_volume_widths(widths)
    with pytest.raises(ValueError, match="16 or a multiple of 32"):
        Fm.fMRIVolumeEncoder3D(widths=widths)


def test_every_accepted_width_meets_each_kernel_limit_it_passes_through():
    """the rule restated from the kernels' own limits: as Cin of mm_conv3d_fwd (16 or % 32), unpadded by cpad (% 16), as
    either side of mm_conv3d_wgrad (% 8), through the pool pass (% 8, <= 1024) and the pooled head (% 16, <= 1024)"""
    for w in range(0, 1100):
        ok = ops.volume_width_ok(w)
        limits = (w > 0 and (w == 16 or w % 32 == 0) and ops.cpad(w) == w and w % 8 == 0 and w <= 1024 and w % 16 == 0)
        assert ok == limits, w
