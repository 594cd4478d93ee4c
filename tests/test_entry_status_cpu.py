"""CPU test of the decode, prefill and token-major attention entries (no GPU):
every one of them, whichever cache form, window / sink variant and element
type its name carries, answers the shared argument errors with the same
status (tests/capi_checks.py entry_status_checks; all returned before any HIP
call)."""
import pytest

import capi_checks as cc
import fa_mi355x

SYMBOLS = [cc.entry_symbol(e) for e in cc.ATTENTION_ENTRIES]


def test_table_covers_every_attention_entry():
    assert len(set(SYMBOLS)) == 78
    prefixes = ("fa_decode", "fa_prefill", "fa_attn_varlen")
    helpers = ("fa_decode_num_splits", "fa_decode_ws_bytes", "fa_attn_varlen_bwd_f16", "fa_attn_varlen_bwd_bf16")
    assert set(SYMBOLS) == {s for s in fa_mi355x.EXPORTED_SYMBOLS if s.startswith(prefixes) and s not in helpers}


@pytest.mark.parametrize("entry", cc.ATTENTION_ENTRIES, ids=SYMBOLS)
def test_argument_statuses(entry):
    cc.entry_status_checks(fa_mi355x, fa_mi355x.load_library(), entry)
