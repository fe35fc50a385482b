# Builds tests/_build/gather_print: the rules of device/zmx_gather.h as a plain C++ program (gather_print.cc).
# SANITIZE="-fsanitize=address,undefined" OUT_NAME=gather_print_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
OUT  := $(ROOT)/tests/_build
OUT_NAME ?= gather_print

$(OUT)/$(OUT_NAME): gather_print.cc $(DEV)/zmx_gather.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(DEV) -o $@ gather_print.cc
