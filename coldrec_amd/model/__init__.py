"""Model registry with the reference's shape (model/__init__.py:28-55): name -> trainer class.

Only the hot-path trainers are built in; they are imported lazily so that a missing optional
dependency of some other plugin can never break ``--model MF``.  A stock ColdRec model file that
subclasses ``BaseColdStartTrainer`` can be registered with ``register(name, cls)``.

``keys()`` lists the core trainers plus whatever ``register()`` added, ``names()`` those and the contrastive trainers
(both listings are pinned).  Every other built-in trainer resolves by name through ``[]``, ``.get()`` and ``in`` from one
lazy table with a cache of its own, so resolving one never changes a listing.  ``resolvable()`` is everything a
``--model`` flag can name.
"""
import importlib

_BUILTIN = {'MF': ('.MF', 'MF'), 'LightGCN': ('.LightGCN', 'LightGCN'), 'DropoutNet': ('.DropoutNet', 'DropoutNet')}
_CONTRASTIVE = ('SimGCL', 'XSimGCL')
_LAZY = {name: ('.' + name, name) for name in _CONTRASTIVE + ('CLCRec', 'CCFCRec', 'ALDI', 'GAR', 'NCL', 'NGCF', 'MTPR', 'VBPR',
                                                                   'AMR', 'MetaEmbedding', 'DeepMusic', 'DUIF')}
_lazy_cache = {}


class _Registry(dict):
    def __missing__(self, name):
        if name in _LAZY:                             # kept out of the dict's own storage (see the module docstring)
            if name not in _lazy_cache:
                mod, cls = _LAZY[name]
                _lazy_cache[name] = getattr(importlib.import_module(mod, __name__), cls)
            return _lazy_cache[name]
        if name not in _BUILTIN:
            raise KeyError(name)
        mod, cls = _BUILTIN[name]
        self[name] = getattr(importlib.import_module(mod, __name__), cls)
        return self[name]

    def get(self, name, default=None):
        try:
            return self[name]
        except KeyError:
            return default

    def __contains__(self, name):
        return name in _BUILTIN or name in _LAZY or dict.__contains__(self, name)

    def keys(self):
        return sorted(set(_BUILTIN) | set(dict.keys(self)))

    def names(self):
        """Every model name that resolves: core + contrastive + registered."""
        return sorted(set(_BUILTIN) | set(_CONTRASTIVE) | set(dict.keys(self)))

    def resolvable(self):
        """Everything a ``--model`` flag can name: ``names()`` + the rest of the lazy table."""
        return sorted(set(self.names()) | set(_LAZY))


AVAILABLE_MODELS = _Registry()


def resolvable():
    return AVAILABLE_MODELS.resolvable()


def register(name, cls):
    AVAILABLE_MODELS[name] = cls
