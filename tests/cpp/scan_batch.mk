# reduce_batch.mk (./Makefile's programs + the C++ API tests of the batched sort and the batched reduce) plus the C++ API test of
# the batched scan (test_batch_scan_api.cpp), through the same variables and pattern rule:
#   make -C tests/cpp -f scan_batch.mk
include reduce_batch.mk
.DEFAULT_GOAL := with_scan_batch
with_scan_batch: with_reduce_batch $(BIN)/test_batch_scan_api
.PHONY: with_scan_batch
