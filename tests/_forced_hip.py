"""The real HIP back end with chosen answers: ``kernels.HipKernels`` whose route questions
(``*_supported``, ``pw_wgrad_tiled``, ``blend_backward_writes_table``) can be turned from the
library's "yes" into a "no", so that the fall-back branches of the fused MLP chains
(``mmdet3d_ops/fused_mlp.py``) run on the device with real numbers.

It takes the same ``answers`` table as ``tests/_launch_recorder.LaunchRecorder``:
{question: bool or callable(*args) -> bool}.  An answer can only REFUSE: every question returns
``real(*args) and forced(*args)``, so every launch that then happens is one the library accepts for
that shape -- nothing is ever forced onto a kernel that would refuse it.

``launched`` lists the names of the methods that were called, questions left out, in order."""
import contextlib

from nesie_amd import kernels
from nesie_amd.kernels import HipKernels

_QUESTIONS = ('pw_wgrad_tiled', 'blend_backward_writes_table')
# host-side size queries: no launch
_QUIET = ('pw_stat_slots', 'mlp_stream_parts', 'cu_budget')


def _is_question(method):
    return method.endswith('_supported') or method in _QUESTIONS


class ForcedHip(HipKernels):
    name = 'hip'

    def __init__(self, answers=None):
        self.answers = dict(answers or {})
        for q in self.answers:
            assert _is_question(q) and hasattr(HipKernels, q), f'{q} is no route question of HipKernels'
        self.launched = []

    def __getattribute__(self, method):
        value = object.__getattribute__(self, method)
        if method.startswith('_') or not callable(value) or method in ('answers', 'launched'):
            return value
        if _is_question(method):
            forced = object.__getattribute__(self, 'answers').get(method, True)

            def ask(*args):
                return bool(value(*args)) and bool(forced(*args) if callable(forced) else forced)
            return ask
        if method in _QUIET or not hasattr(HipKernels, method):
            return value

        def launch(*args, **kwargs):
            self.launched.append(method)
            return value(*args, **kwargs)
        return launch


@contextlib.contextmanager
def forced_hip(answers=None):
    """Run the enclosed code with a ``ForcedHip`` serving every op; -> the back end."""
    with kernels.use_backend(ForcedHip(answers)) as backend:
        yield backend
