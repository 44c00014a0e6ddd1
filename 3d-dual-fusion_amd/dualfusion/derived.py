"""Values derived from parameters and buffers (packed filters, folded BatchNorm, concatenated weights, launch tables), kept
with the object they belong to and rebuilt when a tensor they were built from changes.  Host-side only."""


def tensors_key(tensors):
    """The cache key of something derived from `tensors` (None allowed): address, version counter, device and dtype of each.
    Host-side only.  In-place updates under no_grad (optimizers, load_state_dict, `bn.bias.add_()`) move the version,
    re-seated or converted storage moves the address; writes through `.data` move neither and are not tracked."""
    return tuple(None if t is None else (t.data_ptr(), t._version, t.device, t.dtype) for t in tensors)


def state_slots(module):
    """[(dict, name)] of every parameter and buffer of the module tree, to be collected ONCE (the tree walk is host time per
    step) and read with `slot_tensors` per call: the modules' own `_parameters` / `_buffers` dicts always hold the live
    objects, also after `.double().float()` or an assignment replaced a buffer -- a list of the tensors themselves would go
    on watching the dead ones."""
    return [(d, k) for m in module.modules() for d in (m._parameters, m._buffers) for k in d]


def slot_tensors(slots):
    return [d.get(k) for d, k in slots]


def derived(cache, name, tensors, build, extra=()):
    """cache[name] = (key, value): what `build()` derives from `tensors`, rebuilt when tensors_key(tensors) or `extra` changes.
    `cache` is the __dict__ of the object the value belongs to (a module, a parameter), so the value dies with its owner.
    `tensors` are the parameters and buffers themselves, never a view or a copy computed per call."""
    key = (tensors_key(tensors), extra)
    hit = cache.get(name)
    if hit is None or hit[0] != key:
        hit = cache[name] = (key, build())
    return hit[1]
