"""The binding's one tensor check (vimg_amd.hip._device_tensor) on what it refuses before anything reaches the GPU:
a wrong dtype, a wrong shape, and a value that is neither a numpy array nor a CUDA tensor raise ValueError with the
words the GPU tests match on, nothing is copied up, and CUDA is not initialised (on a machine without a GPU
initialising it would raise another error, so the assertion checks itself)."""
import numpy as np
import pytest
import torch

from vimg_amd import hip

F32 = ("float32",)
MASK = ("uint8", "bool")

REFUSED = {
    "numpy float64": (lambda: np.zeros((4, 8), np.float64), F32, (None, 8), "float32"),
    "numpy shape, fixed rows and cols": (lambda: np.zeros((5, 3), np.float32), F32, (6, 3), "shape"),
    "numpy shape, open N": (lambda: np.zeros((4, 7), np.float32), F32, (None, 8), "shape"),
    "numpy shape, open N, one dimension short": (lambda: np.zeros(8, np.float32), F32, (None, 8), "shape"),
    "python list": (lambda: [[0.0] * 8] * 4, F32, (None, 8), "expected a torch CUDA tensor or a numpy array"),
    "cpu tensor": (lambda: torch.zeros((4, 4)), F32, (None, 4), "CUDA device"),
    "int32 mask": (lambda: np.zeros((20, 36), np.int32), MASK, (20, 36), "uint8 or bool"),
    "int32 tensor mask": (lambda: torch.zeros((20, 36), dtype=torch.int32), MASK, (20, 36), "uint8 or bool"),
}


@pytest.fixture
def no_upload(monkeypatch):
    """Any copy to the GPU fails the test; tells afterwards whether CUDA was initialised on the way."""
    def refuse(a):
        raise AssertionError("the value was copied up before it was checked")
    monkeypatch.setattr(hip, "_upload", refuse)
    before = torch.cuda.is_initialized()
    yield
    assert torch.cuda.is_initialized() == before, "the check initialised CUDA"


@pytest.mark.parametrize("case", list(REFUSED))
@pytest.mark.parametrize("aligned", [False, True])
def test_refused_before_the_gpu_is_touched(case, aligned, no_upload):
    make, dtypes, shape, word = REFUSED[case]
    with pytest.raises(ValueError, match=word) as e:
        hip._device_tensor(make(), "arg", dtypes, shape, aligned=aligned)
    assert str(e.value).startswith("arg: ")


def test_an_output_buffer_is_refused_in_one_sentence(no_upload):
    for out in (np.zeros((4, 4), np.float32), torch.zeros((4, 4)), torch.zeros((4, 4), dtype=torch.float64), [1.0]):
        with pytest.raises(ValueError, match=r"out must be a contiguous torch.float32 CUDA tensor of shape \(4, 4\)"):
            hip._device_tensor(out, "trace_rays", F32, (4, 4), aligned=True, out=True)


POST_REFUSED = {
    "cpu tensor": (lambda: torch.zeros((4, 8, 3)), 1, "post_rgb8 image: the tensor must be on the current CUDA device"),
    "float64 tensor": (lambda: torch.zeros((4, 8, 3), dtype=torch.float64), 1, "post_rgb8 image: dtype must be float32, not torch.float64"),
    "float64 numpy": (lambda: np.zeros((4, 8, 3), np.float64), 1, "post_rgb8 image: dtype must be float32, not float64"),
    "non-contiguous view": (lambda: torch.zeros((8, 4, 3)).transpose(0, 1), 1, "post_rgb8 image: the tensor must be"),
    "four channels": (lambda: np.zeros((4, 8, 4), np.float32), 1, r"post_rgb8 image: shape must be \(H, W, 3\), not \(4, 8, 4\)"),
    "four channels, tensor": (lambda: torch.zeros((4, 8, 4)), 1, r"post_rgb8 image: shape must be \(H, W, 3\), not \(4, 8, 4\)"),
    "no rows": (lambda: np.zeros((0, 8, 3), np.float32), 1, r"post_rgb8 image: shape must be \(H, W, 3\), not \(0, 8, 3\)"),
    "python list": (lambda: [[[0.0] * 3] * 8] * 4, 1, "post_rgb8 image: shape must be"),
    "operator 4": (lambda: np.zeros((4, 8, 3), np.float32), 4, "post_rgb8: tonemapper must be 0 .* not 4"),
    "operator -1": (lambda: np.zeros((4, 8, 3), np.float32), -1, "post_rgb8: tonemapper must be 0 .* not -1"),
    "operator 1.5": (lambda: np.zeros((4, 8, 3), np.float32), 1.5, "post_rgb8: tonemapper must be 0 .* not 1.5"),
}


@pytest.mark.parametrize("case", list(POST_REFUSED))
def test_post_rgb8_refuses_before_the_gpu_is_touched(case, no_upload, monkeypatch):
    """hip.post_rgb8 goes through the same check as every other launch: nothing is copied, CUDA is not initialised
    and the library is not called (it is not even loaded)."""
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(hip, "_lib", no_library)
    make, tonemapper, words = POST_REFUSED[case]
    with pytest.raises(ValueError, match=words):
        hip.post_rgb8(make(), tonemapper)


def test_a_numpy_bool_mask_passes_the_host_checks_and_goes_up_as_uint8(monkeypatch):
    sent = []

    def upload(a):
        sent.append(a)
        return torch.from_numpy(a)       # (stays on the host: the checks before the copy are what is tested)
    monkeypatch.setattr(hip, "_upload", upload)
    before = torch.cuda.is_initialized()
    mask = np.zeros((20, 36), dtype=bool)[:, ::-1]      # not contiguous: made so on the way
    mask[3, 5] = True
    t, host = hip._device_tensor(mask, "mask", MASK, (20, 36))
    assert host and len(sent) == 1
    assert sent[0].dtype == np.uint8 and sent[0].flags["C_CONTIGUOUS"] and sent[0].shape == (20, 36)
    assert np.array_equal(sent[0], mask.astype(np.uint8))
    assert t.dtype == torch.uint8 and tuple(t.shape) == (20, 36)
    hip._device_tensor(np.zeros((20, 36), np.uint8), "mask", MASK, (20, 36))
    hip._device_tensor(np.zeros((7, 8), np.float32), "rays", F32, (None, 8), aligned=True)
    assert len(sent) == 3 and torch.cuda.is_initialized() == before
