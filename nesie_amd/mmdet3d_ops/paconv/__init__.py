"""Mirror of ``mmdet3d/ops/paconv``: the position-adaptive convolution of PAConv
(arXiv 2103.14635) -- ``assign_score_withk`` on HIP kernels, ``PAConv`` in torch ops and
``PAConvCUDA`` on the kernel.  ``from nesie_amd.mmdet3d_ops.paconv import PAConv,
assign_score_withk`` is the supported spelling (see the note in ``mmdet3d_ops/__init__.py``)."""
from .assign_score import assign_score_withk
from .paconv import PAConv, PAConvCUDA

__all__ = ['assign_score_withk', 'PAConv', 'PAConvCUDA']
