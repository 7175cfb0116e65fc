# batch.mk (./Makefile's programs + the C++ API test of the batched sort) plus the C++ API test of the batched reduce
# (test_batch_reduce_api.cpp), through the same variables and pattern rule:
#   make -C tests/cpp -f reduce_batch.mk
include batch.mk
.DEFAULT_GOAL := with_reduce_batch
with_reduce_batch: with_batch $(BIN)/test_batch_reduce_api
.PHONY: with_reduce_batch
