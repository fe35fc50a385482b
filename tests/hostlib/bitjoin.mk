# Builds tests/_build/bitjoin_print: the rules of device/zmx_bitjoin.h as a plain C++ program (bitjoin_print.cc), and
# tests/_build/bitjoin_checks: the argument rules of zmx_bitjoin_device (host/entry_checks.h) on tables from stdin.
# SANITIZE="-fsanitize=address,undefined" OUT_NAME=bitjoin_print_san builds the first with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
OUT_NAME ?= bitjoin_print

all: $(OUT)/$(OUT_NAME) $(OUT)/bitjoin_checks
.PHONY: all

$(OUT)/$(OUT_NAME): bitjoin_print.cc $(DEV)/zmx_bitjoin.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(DEV) -o $@ bitjoin_print.cc

$(OUT)/bitjoin_checks: bitjoin_checks.cc $(HOST)/entry_checks.h $(HOST)/device_output_plan.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra -I$(ROOT)/include -I$(HOST) -o $@ bitjoin_checks.cc
