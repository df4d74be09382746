"""Containers of the sparse layers (the role of ``mmdet3d/ops/spconv/modules.py``)."""
from collections import OrderedDict

from torch import nn

from .structure import SparseConvTensor


class SparseModule(nn.Module):
    """Marker: a ``SparseSequential`` hands a subclass the ``SparseConvTensor`` itself, any
    other module the feature matrix."""


def is_spconv_module(module):
    return isinstance(module, SparseModule)


def is_sparse_conv(module):
    from .conv import SparseConvolution
    return isinstance(module, SparseConvolution)


class SparseSequential(SparseModule):
    """A sequential container: modules in positional order, or one ``OrderedDict``, or keywords
    (``SparseSequential(conv1=SubMConv3d(...), relu1=nn.ReLU())``)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], OrderedDict):
            for key, module in args[0].items():
                self.add_module(key, module)
        else:
            for idx, module in enumerate(args):
                self.add_module(str(idx), module)
        for name, module in kwargs.items():
            if name in self._modules:
                raise ValueError('name exists.')
            self.add_module(name, module)
        self._sparity_dict = {}

    def __getitem__(self, idx):
        if not (-len(self) <= idx < len(self)):
            raise IndexError('index {} is out of range'.format(idx))
        return list(self._modules.values())[idx]

    def __len__(self):
        return len(self._modules)

    @property
    def sparity_dict(self):
        return self._sparity_dict

    def add(self, module, name=None):
        if name is None:
            name = str(len(self._modules))
            if name in self._modules:
                raise KeyError('name exists')
        self.add_module(name, module)

    def forward(self, input):
        for k, module in self._modules.items():
            if is_spconv_module(module):
                assert isinstance(input, SparseConvTensor)
                self._sparity_dict[k] = input.sparity
                input = module(input)
            elif isinstance(input, SparseConvTensor):
                if input.indices.shape[0] != 0:
                    input.features = module(input.features)
            else:
                input = module(input)
        return input

    def fused(self):
        raise NotImplementedError(
            'SparseSequential.fused: folding BatchNorm into the sparse conv is not built '
            '(fused_bn layers are outside this build)')


class ToDense(SparseModule):
    """SparseConvTensor -> dense (B, C, D, H, W)."""

    def forward(self, x: SparseConvTensor):
        return x.dense()


class RemoveGrid(SparseModule):
    """Drops a pre-allocated grid buffer."""

    def forward(self, x: SparseConvTensor):
        x.grid = None
        return x
