"""Model registry with the reference's shape (model/__init__.py:28-55): name -> trainer class.

Only the hot-path trainers are built in; they are imported lazily so that a missing optional
dependency of some other plugin can never break ``--model MF``.  A stock ColdRec model file that
subclasses ``BaseColdStartTrainer`` can be registered with ``register(name, cls)``.

``keys()`` lists the core trainers plus whatever ``register()`` added.  The contrastive trainers (SimGCL, XSimGCL)
resolve by name through ``[]``, ``.get()`` and ``in`` as well, from a cache of their own: resolving one never changes
what ``keys()`` reports.  The cold-start trainers CLCRec, CCFCRec, ALDI and GAR resolve the same way from a third table and are not part of
``names()`` either (both listings are pinned); NCL, the third graph-contrastive backbone, has a fourth table for the same
reason, NGCF, the third warm backbone, a fifth, and MTPR a sixth.  ``resolvable()`` is everything a ``--model`` flag can name.
"""
import importlib

_BUILTIN = {'MF': ('.MF', 'MF'), 'LightGCN': ('.LightGCN', 'LightGCN'), 'DropoutNet': ('.DropoutNet', 'DropoutNet')}
_CONTRASTIVE = {'SimGCL': ('.SimGCL', 'SimGCL'), 'XSimGCL': ('.XSimGCL', 'XSimGCL')}
_COLD = {'CLCRec': ('.CLCRec', 'CLCRec'), 'CCFCRec': ('.CCFCRec', 'CCFCRec'), 'ALDI': ('.ALDI', 'ALDI'),
         'GAR': ('.GAR', 'GAR')}
_NCL = {'NCL': ('.NCL', 'NCL')}
_NGCF = {'NGCF': ('.NGCF', 'NGCF')}
_MTPR = {'MTPR': ('.MTPR', 'MTPR')}
_contrastive_cache = {}
_cold_cache = {}
_ncl_cache = {}
_ngcf_cache = {}
_mtpr_cache = {}


class _Registry(dict):
    def __missing__(self, name):
        if name in _CONTRASTIVE:                      # kept out of the dict's own storage (see the module docstring)
            if name not in _contrastive_cache:
                mod, cls = _CONTRASTIVE[name]
                _contrastive_cache[name] = getattr(importlib.import_module(mod, __name__), cls)
            return _contrastive_cache[name]
        if name in _COLD:
            if name not in _cold_cache:
                mod, cls = _COLD[name]
                _cold_cache[name] = getattr(importlib.import_module(mod, __name__), cls)
            return _cold_cache[name]
        if name in _NCL:
            if name not in _ncl_cache:
                mod, cls = _NCL[name]
                _ncl_cache[name] = getattr(importlib.import_module(mod, __name__), cls)
            return _ncl_cache[name]
        if name in _NGCF:
            if name not in _ngcf_cache:
                mod, cls = _NGCF[name]
                _ngcf_cache[name] = getattr(importlib.import_module(mod, __name__), cls)
            return _ngcf_cache[name]
        if name in _MTPR:
            if name not in _mtpr_cache:
                mod, cls = _MTPR[name]
                _mtpr_cache[name] = getattr(importlib.import_module(mod, __name__), cls)
            return _mtpr_cache[name]
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
        return name in _BUILTIN or name in _CONTRASTIVE or name in _COLD or name in _NCL or name in _NGCF or \
            name in _MTPR or dict.__contains__(self, name)

    def keys(self):
        return sorted(set(_BUILTIN) | set(dict.keys(self)))

    def names(self):
        """Every model name that resolves: core + contrastive + registered."""
        return sorted(set(_BUILTIN) | set(_CONTRASTIVE) | set(dict.keys(self)))

    def resolvable(self):
        """Everything a ``--model`` flag can name: ``names()`` + the cold-start trainers + NCL + NGCF + MTPR."""
        return sorted(set(self.names()) | set(_COLD) | set(_NCL) | set(_NGCF) | set(_MTPR))


AVAILABLE_MODELS = _Registry()


def resolvable():
    return AVAILABLE_MODELS.resolvable()


def register(name, cls):
    AVAILABLE_MODELS[name] = cls
