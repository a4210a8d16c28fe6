"""``EditSession._atomic`` on the device: the flag protocol every atomic session operation runs on (fold, release, refold, rescale /
reweight), with a stand-in for the launches — a non-zero flag word undoes once, zeroes the word and raises with the code handed to
``refuse``; a zero one returns.  No kernel of the library is launched.
Run on the MI355X box:  python -m pytest tests/test_session_module_gpu.py -m gpu -q"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import edit_session as es

DEV = "cuda:0"


def test_a_nonzero_flag_undoes_once_zeroes_the_word_and_raises():
    info = torch.full((1,), 3, dtype=torch.int32, device=DEV)       # (stale: _atomic zeroes the word before it launches)
    seen, undone, codes = [], [], []

    def launch():
        seen.append(int(info.item()))
        info.fill_(7)

    def refuse(code):
        codes.append(code)
        return f"refused at column {code - 1}"

    with pytest.raises(torch.linalg.LinAlgError, match="refused at column 6"):
        es.EditSession._atomic(info, launch, lambda: undone.append(int(info.item())), refuse)
    assert seen == [0] and undone == [7] and codes == [7] and int(info.item()) == 0


def test_a_zero_flag_returns_without_undoing():
    info = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    ran, undone = [], []
    assert es.EditSession._atomic(info, lambda: ran.append(1), lambda: undone.append(1), lambda code: "never") is None
    assert ran == [1] and undone == [] and int(info.item()) == 0


def test_a_second_flag_word_is_read_with_the_first():
    info, also = torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((1,), 5, dtype=torch.int32, device=DEV)
    undone, codes = [], []
    with pytest.raises(torch.linalg.LinAlgError):
        es.EditSession._atomic(info, lambda: None, lambda: undone.append(1), lambda code: codes.append(code) or "no", also=also)
    assert undone == [1] and codes == [5] and int(info.item()) == 0 and int(also.item()) == 5
