"""Every array of the library's grid buffer (dsdf_pad_grid; the table in include/dsdf.h) read back from the device and compared,
exactly, with numpy brute force at offsets written out from that table (tests/grid_buffer_cases.py): the clamped padded copy, the
dilated block minima of both levels, the dilated block maxima, the 6^3 window maxima and minima, the third stage's gradient bound D
and every float of the row-block copy.  The undilated block arrays are scratch and not asserted."""
import numpy as np
import pytest

from grid_buffer_cases import GRIDS, layout, noise, reference


@pytest.mark.parametrize('dims', GRIDS)
def test_offsets_sum_to_the_padded_size(built, dims):
    import dsdf
    arrays, total = layout(dims)
    assert total == dsdf.load().dsdf_padded_size(*dims)
    assert arrays['rows'][0] % 4 == 0
    ref = reference(dims)
    assert all(ref[k].shape == arrays[k][1] and ref[k].dtype == np.float32 for k in ref if k != 'D')


@pytest.mark.gpu
@pytest.mark.parametrize('dims', GRIDS)
def test_grid_buffer_equals_brute_force(built, dims):
    import dsdf
    import torch
    dsdf.load()
    buf = dsdf.SdfGrid(torch.from_numpy(noise(dims).copy()).cuda()).padded.cpu().numpy()
    arrays, total = layout(dims)
    assert buf.size == total and buf.dtype == np.float32
    ref = reference(dims)
    for name, want in ref.items():
        if name == 'D':
            continue
        off, shape = arrays[name]
        got = buf[off:off + want.size].reshape(shape)
        assert (got == want).all(), f"{name}: {int((got != want).sum())} of {want.size} floats differ"
    if ref['D'] is not None:          # (2,2,2) has one block of maxima: no gradient bound, and nothing said about those floats
        off = arrays['max_raw'][0]
        assert buf[off:off + 3].tolist() == ref['D'].tolist()
