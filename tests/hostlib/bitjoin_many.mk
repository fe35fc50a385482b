# Builds tests/_build/bitjoin_many_print: the rules of k_bitjoin_many (device/zmx_bitjoin.h) as a plain C++ program
# (bitjoin_many_print.cc), and tests/_build/bitjoin_many_checks: the argument rules of zmx_bitjoin_many_device
# (host/entry_checks.h) and the packed form's arithmetic (host/device_output_plan.h) on tables from the command line.
# SANITIZE="-fsanitize=address,undefined" OUT_NAME=bitjoin_many_print_san builds the first with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
OUT_NAME ?= bitjoin_many_print

all: $(OUT)/$(OUT_NAME) $(OUT)/bitjoin_many_checks
.PHONY: all

$(OUT)/$(OUT_NAME): bitjoin_many_print.cc $(DEV)/zmx_bitjoin.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(DEV) -o $@ bitjoin_many_print.cc

$(OUT)/bitjoin_many_checks: bitjoin_many_checks.cc $(HOST)/entry_checks.h $(HOST)/device_output_plan.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra -I$(ROOT)/include -I$(HOST) -o $@ bitjoin_many_checks.cc
