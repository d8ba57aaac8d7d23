"""XSimGCL warm-embedding trainer on the MI355X (reference: model/XSimGCL.py).

One perturbed propagation per batch serves both losses: BPR on the mean of the layers, InfoNCE between that mean and the
output of layer ``--l_cl`` (model/XSimGCL.py:30-34,58-63,106-124).  The step is ``train.CLEngine(mode='xsimgcl')``.
"""
from .SimGCL import SimGCL, SimGCL_Encoder


class XSimGCL_Encoder(SimGCL_Encoder):
    """Xavier tables (user first, model/XSimGCL.py:98-104) + the contrastive layer."""

    def __init__(self, args, data, emb_size, n_layers, device):
        super().__init__(args, data, emb_size, n_layers, device)
        self.layer_cl = args.l_cl


class XSimGCL(SimGCL):
    cl_mode = 'xsimgcl'

    def __init__(self, config):
        a = config.args
        if not (1 <= a.l_cl <= a.layers):
            raise ValueError(
                "XSimGCL requires 1 <= l_cl <= layers (contrastive snapshot at GCN layer l_cl); "
                f"got l_cl={a.l_cl}, layers={a.layers}."
            )
        super().__init__(config)

    def _make_encoder(self):
        return XSimGCL_Encoder(self.args, self.data, self.emb_size, self.n_layers, self.device)
