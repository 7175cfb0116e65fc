# key_runs.mk (./Makefile's programs + the C++ API tests of the batched sort, reduce and scan and of key runs) plus the C++ API
# test of select (test_select_api.cpp), through the same variables and pattern rule:
#   make -C tests/cpp -f select.mk
include key_runs.mk
.DEFAULT_GOAL := with_select
with_select: with_key_runs $(BIN)/test_select_api
.PHONY: with_select
