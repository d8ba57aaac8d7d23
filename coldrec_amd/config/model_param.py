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


def _lr_wd_pair(v):
    """An (lr, weight decay) pair written as "0.05,0" or as "[0.05, 0]" (brackets or parentheses, spaces allowed)."""
    if isinstance(v, (list, tuple)):
        parts = list(v)
    else:
        parts = str(v).strip().strip('[]()').split(',')
    try:
        if len(parts) != 2:
            raise ValueError
        return [float(x) for x in parts]
    except (TypeError, ValueError):
        raise argparse.ArgumentTypeError(f'expected two numbers such as "0.05,0" or "[0.05, 0]", got {v!r}') from None


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
    if model_name == 'NCL':      # config/model_param.py:318-324
        parser.add_argument('--tau', type=float, default=0.2, help='Contrast temperature')
        parser.add_argument('--ssl_reg', type=float, default=1e-6, help='Weight of the structure contrast')
        parser.add_argument('--proto_reg', type=float, default=1e-7, help='Weight of the prototype contrast')
        parser.add_argument('--alpha', type=float, default=1.0, help='Weight of the item side of the structure contrast')
        parser.add_argument('--hyper_layers', type=int, default=1,
                            help='The context is GCN layer 2 * hyper_layers; needs hyper_layers * 2 <= layers')
        parser.add_argument('--num_clusters', type=int, default=20, help='Prototypes (k-means clusters) per table')
        parser.add_argument('--proto_start', type=int, default=20,
                            help='(addition) first epoch, 0-based, of the prototype phase; the reference hard-codes 20')
    if model_name == 'CLCRec':      # config/model_param.py:125-129
        parser.add_argument('--num_neg', type=int, default=128, help='Sampled negatives per record')
        parser.add_argument('--temp_value', type=float, default=2.0, help='Contrastive loss temperature')
        parser.add_argument('--lr_lambda', type=float, default=0.5, help='Weight of the embedding-content contrastive loss')
        parser.add_argument('--num_sample', type=float, default=0.5,
                            help='Share of the batch rows (drawn with replacement) scored on content instead of embedding')
    if model_name == 'CCFCRec':      # config/model_param.py:130-144
        parser.add_argument('--positive_number', type=int, default=5, help='Contrast positives per record')
        parser.add_argument('--negative_number', type=int, default=40, help='Contrast negatives per positive')
        parser.add_argument('--self_neg_number', type=int, default=40, help='Self-contrast negatives per record')
        parser.add_argument('--tau', type=float, default=0.1, help='Contrast loss temperature')
        parser.add_argument('--lambda1', type=float, default=0.6, help='Weight of the two contrast losses')
        parser.add_argument('--attr_present_dim', type=int, default=64, help='Width of the attribute embeddings')
        parser.add_argument('--implicit_dim', type=int, default=64, help='Width of the user / item tables')
        parser.add_argument('--cat_implicit_dim', type=int, default=64, help='Hidden width of the generator')
        parser.add_argument('--pretrain', type=_str2bool, default=False, nargs='?', const=True,
                            help='Load both tables from ./emb/{dataset}_cold_item_{backbone}_{user,item}_emb.pt')
        parser.add_argument('--pretrain_update', type=_str2bool, default=False, nargs='?', const=True,
                            help='With --pretrain: train the loaded tables (true) or keep them frozen (false)')
    if model_name == 'ALDI':      # config/model_param.py:82-93
        parser.add_argument('--alpha', type=float, default=0.9, help='Weight of the ranking distillation loss')
        parser.add_argument('--beta', type=float, default=0.05, help='Weight of the identification distillation loss')
        parser.add_argument('--gamma', type=float, default=0.1, help='Weight of the rating distillation loss')
        parser.add_argument('--tws', type=int, default=0, choices=[0, 1],
                            help='1: weight the two distillation losses by the positive item\'s frequency')
        parser.add_argument('--freq_coef_M', type=float, default=4, help='Cap of the frequency weights: tanh(M)')
        parser.add_argument('--aldi_hidden', type=int, default=200, help='Hidden width of the two student towers')
    if model_name == 'GAR':       # config/model_param.py:94-96
        parser.add_argument('--alpha', type=float, default=0.05, help='Weight of the similarity term in the generator loss')
        parser.add_argument('--beta', type=float, default=0.1, help='Weight of the sampled negative in the recommender loss')
    if model_name == 'MTPR':      # config/model_param.py:300-303
        parser.add_argument('--p_emb', type=_lr_wd_pair, default=[0.05, 0.0], help='lr and weight decay of the two id tables')
        parser.add_argument('--p_ctx', type=_lr_wd_pair, default=[0.05, 0.01],
                            help='lr and weight decay of the content projection W and of weu')
        parser.add_argument('--p_proj', type=_lr_wd_pair, default=[0.05, 0.01], help='lr and weight decay of wei')
    if model_name in ('VBPR', 'AMR'):      # config/model_param.py:292-299
        parser.add_argument('--p_emb', type=_lr_wd_pair, default=[0.05, 0.0], help='lr and weight decay of the three id tables')
        parser.add_argument('--p_ctx', type=_lr_wd_pair, default=[0.05, 0.01], help='lr and weight decay of the content projection W')
    if model_name == 'AMR':
        parser.add_argument('--eps', type=float, default=0.1, help='Length of the adversarial shift of a content row')
        parser.add_argument('--lmd', type=float, default=1, help='Weight of the adversarial term')
    if model_name == 'MetaEmbedding':      # config/model_param.py:266-267 (DeepMusic takes no flags of its own)
        parser.add_argument('--alpha', type=float, default=0.5,
                            help='Weight of the cold-start loss; 1 - alpha weighs the warm-up loss')
    return parser
