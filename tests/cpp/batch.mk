# ./Makefile plus the C++ API test of the batched sort (test_batch_sort_api.cpp), through the same variables and pattern rule:
#   make -C tests/cpp -f batch.mk
include Makefile
.DEFAULT_GOAL := with_batch
with_batch: all $(BIN)/test_batch_sort_api
.PHONY: with_batch
