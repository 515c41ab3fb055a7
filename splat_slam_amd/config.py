"""The reference's YAML configs as one dict (the semantics of its load_config / update_recursive / save_config).

    load_config(path, default_path=None, root=None) -> dict
        The file at `path`, laid over what it inherits: its `inherit_from` names another file, which is loaded the same way first
        (recursively), and the file at the end of that chain is laid over `default_path` when one is given.  Nested dicts merge key by
        key; scalars and lists are replaced.  An `inherit_from` path is used as written, i.e. relative to the current directory as in
        the reference, unless `root` is given: then a relative one is resolved against `root` (the directory the configs were
        written for, e.g. a checkout whose files say `configs/Replica/replica.yaml`).  `path` and `default_path` themselves are the
        caller's and are opened as given.
    update_recursive(dst, src)      lays src over dst in place (returns dst)
    save_config(cfg, path)          YAML; load_config(path) gives an equal dict back
"""
import os

import yaml

__all__ = ["load_config", "update_recursive", "save_config"]


def _read(path):
    with open(path, "r") as f:
        cfg = yaml.safe_load(f)
    if cfg is None:
        return {}
    if not isinstance(cfg, dict):
        raise ValueError(f"{path}: a config file holds a mapping, not {type(cfg).__name__}")
    return cfg


def update_recursive(dst, src):
    for key, value in src.items():
        if isinstance(value, dict):
            if not isinstance(dst.get(key), dict):
                dst[key] = {}
            update_recursive(dst[key], value)
        else:
            dst[key] = value
    return dst


def load_config(path, default_path=None, root=None):
    own = _read(path)
    parent = own.get("inherit_from")
    if parent is not None:
        if root is not None and not os.path.isabs(parent):
            parent = os.path.join(root, parent)
        cfg = load_config(parent, default_path, root)
    elif default_path is not None:
        cfg = _read(default_path)
    else:
        cfg = {}
    return update_recursive(cfg, own)


def save_config(cfg, path):
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
