# scan_batch.mk (./Makefile's programs + the C++ API tests of the batched sort, reduce and scan) plus the C++ API test of key runs
# (test_key_runs_api.cpp), through the same variables and pattern rule:
#   make -C tests/cpp -f key_runs.mk
include scan_batch.mk
.DEFAULT_GOAL := with_key_runs
with_key_runs: with_scan_batch $(BIN)/test_key_runs_api
.PHONY: with_key_runs
