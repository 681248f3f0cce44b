"""What the projector needs of SG3/genlib/utils/util_general.py (:70-74 the default dicts, :242-274 the path helpers).
The IFTTT notifier of that module posts to the network and is left out."""
import collections
import ntpath
import os


def list_dict():
    """A dict whose missing keys start as empty lists (the per-step loss history)."""
    return collections.defaultdict(list)


def nested_dict():
    """A dict of dicts of ... to any depth (projected_w[patient][slice])."""
    return collections.defaultdict(nested_dict)


def plain_dict(d):
    """nested_dict -> plain dicts, so that the pickle needs no class of this package to load."""
    return {k: plain_dict(v) for k, v in d.items()} if isinstance(d, dict) else d


def split_dos_path_into_components(path):
    """'a/b/c.ext' -> ['a', 'b', 'c.ext'] (an absolute path keeps its root as the first component)."""
    parts = []
    while True:
        path, last = os.path.split(path)
        if last:
            parts.append(last)
            continue
        if path:
            parts.append(path)
        break
    return parts[::-1]


def get_filename(path):
    head, tail = ntpath.split(path)
    return tail or ntpath.basename(head)


def get_filename_without_extension(path):
    return os.path.splitext(get_filename(path))[0]


def create_dir(outdir):
    os.makedirs(outdir, exist_ok=True)
