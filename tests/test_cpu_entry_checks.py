"""The entry checks of test_gpu_entry_checks.py against the host test library: its stand-in for the device layer
(tests/hostlib/zmx_oracle_backend.cc) runs the device layer's own rules (csrc/host/entry_checks.h) on its own tables,
for every entry it has (it has no hash links and no DP rows): the same requests are refused, with the same texts and class.  CPU only."""
import pytest

import oracle_lib as ol
import test_gpu_entry_checks as ec


@pytest.fixture(scope="module")
def host_ctx():
    from zopfli_amd import Context
    ctx = Context(0, ol.hosttest_library())
    yield ctx
    ctx.close()


def test_store_refs_checked_host_backend(host_ctx):
    ec.store_refs_checked(host_ctx)


def test_trimmed_tables_refuse_host_backend(host_ctx):
    ec.trimmed_tables_refuse(host_ctx, hash_links=False, dp_rows=False)


def test_matches_only_tables_refuse_host_backend(host_ctx):
    ec.matches_only_tables_refuse(host_ctx, dp_rows=False)
