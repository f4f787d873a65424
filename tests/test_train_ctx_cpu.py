"""The training ctx is addressed by field name: ``train_ctx_fields()`` is the ordered name table expanded from
the same list as ``train::Layer`` / ``train::Args`` and their decoder (csrc/train_ctx.h), and ``pack_ctx`` orders
a dict by it.  Needs the built library, not a GPU."""
import os

import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, train_ops

pytestmark = pytest.mark.skipif(not os.path.exists(_ext.SO_PATH), reason="extension library not built")

N_FIELDS = 6 * 18 + 27


def _names():
    return list(_ext.ops().train_ctx_fields())


def test_field_table():
    names = _names()
    assert len(names) == N_FIELDS and len(set(names)) == N_FIELDS
    assert names[0] == "L0.wf" and names[18] == "L1.wf" and names[6 * 18] == "x" and names[-1] == "hpart"
    assert "bwd_self" not in names  # a launch flag, not a ctx field


def test_pack_ctx_orders_by_name():
    names = _names()
    values = {n: 1000 + 7 * i for i, n in enumerate(names)}
    shuffled = dict(sorted(values.items(), key=lambda kv: hash(kv[0])))  # insertion order must not matter
    ctx = train_ops.pack_ctx(shuffled)
    assert ctx.dtype == torch.int64 and ctx.device.type == "cpu"
    assert ctx.tolist() == [values[n] for n in names]


def test_pack_ctx_names_the_bad_field():
    names = _names()
    values = {n: i for i, n in enumerate(names)}
    missing = dict(values)
    del missing["L3.dZ"]
    with pytest.raises(KeyError, match="L3.dZ"):
        train_ops.pack_ctx(missing)
    with pytest.raises(ValueError, match="no_such_field"):
        train_ops.pack_ctx(dict(values, no_such_field=1))
