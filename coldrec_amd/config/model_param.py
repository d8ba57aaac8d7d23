"""Per-model command line flags (reference: config/model_param.py).  Only the models this package
builds are known here; flags of other ColdRec plugins stay in their own checkout."""
import argparse


def _str2bool(v):
    if isinstance(v, bool):
        return v
    s = str(v).strip().lower()
    if s in ('1', 'true', 't', 'yes', 'y', 'on'):
        return True
    if s in ('0', 'false', 'f', 'no', 'n', 'off'):
        return False
    raise argparse.ArgumentTypeError(f'expected a boolean value, got {v!r}')


def model_specific_param(model_name, parser, available_models):
    if model_name not in available_models:
        names = available_models.resolvable() if hasattr(available_models, 'resolvable') else \
            available_models.names() if hasattr(available_models, 'names') else available_models.keys()
        raise ValueError(f"Invalid model name: {model_name}. Available models: {list(names)}")
    # MF and LightGCN take no flags beyond the common ones (--layers is common, main.py:94)
    if model_name == 'DropoutNet':      # config/model_param.py:242-255
        parser.add_argument('--n_dropout', type=float, default=0.5, help='Dropout rate of the network training')
        parser.add_argument('--dropoutnet_hidden1', type=int, default=200, help='DeepCF first hidden width')
        parser.add_argument('--dropoutnet_hidden2', type=int, default=100, help='DeepCF second hidden width')
    if model_name in ('SimGCL', 'XSimGCL'):      # config/model_param.py:304-317
        parser.add_argument('--cl_rate', type=float, default=0.5, help='Weight of contrastive loss')
        parser.add_argument('--tau', type=float, default=0.2, help='InfoNCE temperature')
        parser.add_argument('--eps', type=float, default=0.1, help='Perturbation scale')
        if model_name == 'XSimGCL':
            parser.add_argument('--l_cl', type=int, default=2,
                                help='1-based GCN layer index of the contrastive branch; must satisfy 1 <= l_cl <= layers.')
        parser.add_argument('--cl_noise', choices=['device', 'host'], default='device',
                            help='(addition) where the perturbation noise comes from: device = generated in the kernel '
                                 '(Philox4x32-10 keyed by --seed); host = torch.rand on the CPU generator, uploaded per '
                                 'layer -- the reference\'s own stream, for parity runs')
    if model_name == 'CLCRec':      # config/model_param.py:125-129
        parser.add_argument('--num_neg', type=int, default=128, help='Sampled negatives per record')
        parser.add_argument('--temp_value', type=float, default=2.0, help='Contrastive loss temperature')
        parser.add_argument('--lr_lambda', type=float, default=0.5, help='Weight of the embedding-content contrastive loss')
        parser.add_argument('--num_sample', type=float, default=0.5,
                            help='Share of the batch rows (drawn with replacement) scored on content instead of embedding')
    return parser
